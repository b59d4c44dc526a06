"""Host side of orthogonalised momentum for the large matrices in FlatAdam (include/avmoe.h: avmoe_opt_muon_large_bytes,
avmoe_opt_muon_large_table_build, avmoe_opt_muon_large_classes, avmoe_opt_muon_step_large, avmoe_opt_muon_ns_large;
avmoe_amd.train.FlatAdam(muon=True, muon_large=True)): the symbols and layouts the binding relies on, the checks and the class grouping
of the image builder, the checks of the two launching calls (they precede any launch: host pointers and a NULL stream are enough, no
GPU is needed), every ValueError of the constructor, the selection rule on a MoEAdapter of each variant, and the fp32 restatement of
the iteration against the bound the device test holds."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import FlatAdam
from tests import muon_ref as R
from tests.golden_util import load_golden
from tests.test_adapters_api import _opt
from tests.test_flat_adam_lamb_api import _buf, _err, _reducer, BAD_ARG, ALIGNMENT
from tests.test_flat_adam_muon_api import VARIANTS, _mats, _ranges
from tests.test_flat_adam_muon_large_gpu import KINDS, NS_FACTOR, NS_SHAPES

WORKSPACE = -4
ENTRY_POINTS = ("avmoe_opt_muon_large_bytes", "avmoe_opt_muon_large_table_build", "avmoe_opt_muon_large_classes", "avmoe_opt_muon_step_large",
                "avmoe_opt_muon_ns_large")


def test_header_declares_and_library_exports_the_entry_points():
    L = _capi.lib()
    header = open(_capi.HEADER_PATH).read()
    for name in ENTRY_POINTS:
        assert name in _capi.exported_symbols() and hasattr(L, name) and name in header, name
    assert L.avmoe_abi_version() == 11
    for struct in ("avmoe_opt_muon_large_layout", "avmoe_opt_muon_class"):
        assert f"typedef struct {struct} " in header, struct
    assert C.sizeof(cm.OptMuonLargeLayout) == 3 * C.sizeof(C.c_size_t) + 8 and C.sizeof(cm.OptMuonClass) == 16
    assert "#define AVMOE_MUON_LARGE_MAX_DIM 2048" in header and FlatAdam.MUON_LARGE_MAX_DIM == 2048
    assert "#define AVMOE_MUON_MAX_DIM 128" in header and FlatAdam.MUON_MAX_DIM == 128      # the small rule is what it was


def test_the_signature_and_the_documents():
    sig = inspect.signature(FlatAdam.__init__).parameters
    assert [sig[k].default for k in ("muon_large", "muon_large_max_numel")] == [False, 1 << 23]
    for name in ("muon_paths", "muon_large_shape_of", "muon_select_paths"):
        assert hasattr(FlatAdam, name), name
    assert inspect.signature(FlatAdam.muon_select).parameters.keys() == {"params", "param_groups", "muon_max_numel"}
    assert "The large matrices" in FlatAdam.__doc__ and "verified on one rank" in FlatAdam.__doc__


BAD_CTOR = [dict(muon_large=True), dict(muon=False, muon_large=True), dict(muon=True, muon_large=1), dict(muon=True, muon_large=None),
            dict(muon=True, muon_large="yes"), dict(muon=True, muon_large=True, muon_large_max_numel=0),
            dict(muon=True, muon_large=True, muon_large_max_numel=1e6), dict(muon=True, muon_large=True, muon_large_max_numel=True),
            dict(muon=True, muon_large_max_numel=1 << 20), dict(muon_large_max_numel=1 << 20), dict(muon=True, muon_large=False, muon_large_max_numel=4096)]


@pytest.mark.parametrize("kw", BAD_CTOR, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD_CTOR])
def test_bad_constructor_arguments_raise_value_error_before_anything_is_touched(kw):
    red, w, b = _reducer()
    ptrs = (w.data_ptr(), b.data_ptr())
    with pytest.raises(ValueError, match="muon_large"):
        FlatAdam(red, **kw)
    assert (w.data_ptr(), b.data_ptr()) == ptrs


def test_a_groups_true_is_accepted_only_where_the_large_path_is_on():
    from avmoe_amd.dp import AdapterGradReducer
    big, b = torch.nn.Parameter(torch.zeros(129, 130)), torch.nn.Parameter(torch.zeros(7))
    red = AdapterGradReducer([big, b])
    ptrs = (big.data_ptr(), b.data_ptr())
    groups = [{"params": [big], "muon": True}]
    with pytest.raises(ValueError, match=r"parameter 0 of shape \(129, 130\).*short side <= 128"):      # the present error, word for word
        FlatAdam(red, muon=True, param_groups=groups)
    with pytest.raises(_capi.AvmoeError):                    # accepted: it gets as far as the buckets (the device path has no CPU fallback)
        FlatAdam(red, muon=True, muon_large=True, param_groups=groups)
    with pytest.raises(ValueError, match=r"parameter 1 of shape \(7,\).*short side <= 2048"):
        FlatAdam(red, muon=True, muon_large=True, param_groups=[{"params": [big, b], "muon": True}])
    with pytest.raises(ValueError, match=r"parameter 0 of shape \(129, 130\).*muon_large_max_numel = 100"):
        FlatAdam(red, muon=True, muon_large=True, muon_large_max_numel=100, param_groups=groups)
    with pytest.raises(ValueError, match="muon"):
        FlatAdam(red, muon=True, muon_large=True, param_groups=[{"params": [big], "muon": 1}])
    assert (big.data_ptr(), b.data_ptr()) == ptrs


def test_the_shapes_the_large_path_takes():
    z = torch.zeros
    f = FlatAdam.muon_large_shape_of
    assert f(z(144, 160, 1, 1)) == (144, 160) and f(z(256, 160)) == (256, 160) and f(z(2048, 2048)) == (2048, 2048)
    assert f(z(2049, 2049)) is None and f(z(2049, 2048)) == (2049, 2048)                # the SHORT side <= 2048
    assert f(z(7)) is None and f(z(())) is None and f(z(0, 4)) is None
    assert f(z(144, 160), max_numel=23039) is None and f(z(144, 160), max_numel=23040) == (144, 160)

    def paths(ps, groups=None, **kw):
        return FlatAdam.muon_select_paths(ps, groups, **kw)
    ps = [z(128, 4096), z(2049, 2049), z(4, 32), z(129, 130), z(5), z(128, 2048), z(1, 1 << 19)]
    assert paths(ps, muon_large=True) == [("large", (128, 4096)), None, ("small", (4, 32)), ("large", (129, 130)), None, ("small", (128, 2048)),
                                          ("large", (1, 1 << 19))]      # declined by the small rule for its numel -> the large path
    assert paths(ps) == [None, None, ("small", (4, 32)), None, None, ("small", (128, 2048)), None]
    assert [None if s is None else s[1] for s in paths(ps)] == FlatAdam.muon_select(ps)
    assert paths(ps, muon_large=True, muon_large_max_numel=(1 << 19) - 1)[0] is None    # a numel above muon_large_max_numel
    assert paths(ps, muon_large=True, muon_large_max_numel=1 << 19)[0] == ("large", (128, 4096))
    assert paths([z(3000, 3000)], muon_large=True) == [None]
    assert paths(ps[:4], [{"params": [ps[3]], "muon": False}], muon_large=True)[3] is None
    assert paths(ps[:1], muon_max_numel=1 << 20, muon_large=True) == [("small", (128, 4096))]      # the small rule stays first


@pytest.mark.parametrize("which", list(VARIANTS))
def test_the_selection_on_each_variant(which):
    """C = 256 with 144 x 160 tokens and a 160-wide other modality: conv_adapter (144 x 160) and fc (256 x 160) go to the large path,
    the experts' samplers, the latent tokens and the router's layers keep the small kernel; gates, norms and biases take Adam"""
    _, cfg, _ = load_golden("ave_train")
    cls, kw = VARIANTS[which]
    m = cls(input_dim=256, output_dim=256, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=_opt(cfg), conv_dim_in=160, conv_dim_out=144,
            linear_in=160, linear_out=256, **kw)
    named = list(m.named_parameters())
    params = [p for _, p in named]
    sel = dict(zip((n for n, _ in named), FlatAdam.muon_select_paths(params, muon_large=True)))
    assert sel["conv_adapter.weight"] == ("large", (144, 160)) and sel["fc.weight"] == ("large", (256, 160))
    small = sorted({n.split("experts.")[-1].split(".", 1)[-1] if "experts." in n else n for n, s in sel.items() if s and s[0] == "small"})
    assert small == sorted(["down_sampler.weight", "up_sampler.weight", "my_tokens", "router.0.weight", "router.2.weight", "router.4.weight"])
    old = FlatAdam.muon_select(params)
    for (n, s), o in zip(sel.items(), old):
        if "gate" in n or ".bn" in n or ".ln_" in n or n.endswith("bias"):
            assert s is None, n
        assert (s is not None and s[0] == "small") == (o is not None) and (o is None or s[1] == o), n      # whatever the small rule takes, it keeps
    assert FlatAdam.muon_select_paths(params, [{"params": [dict(named)["conv_adapter.weight"]], "muon": True}], muon_large=True)[
        [n for n, _ in named].index("conv_adapter.weight")] == ("large", (144, 160))
    with pytest.raises(ValueError, match=r"shape \(144, 160, 1, 1\)"):
        FlatAdam.muon_select_paths(params, [{"params": [dict(named)["conv_adapter.weight"]], "muon": True}])


def _build(rows, ranges="own", n_ranges=4, small=(), image="own", nbytes=8192, mats="own"):
    L = _capi.lib()
    if ranges == "own":
        ranges = _ranges([144 * 160, 7, 256 * 160, 129 * 130])
    raw, img = _buf(8192)
    st = L.avmoe_opt_muon_large_table_build(ranges, n_ranges, _mats(rows) if mats == "own" else mats, len(rows), _mats(small) if small else None,
                                            len(small), img if image == "own" else image, nbytes)
    return st, raw, img


def test_the_image_builder_checks_the_matrices_on_the_host():
    L = _capi.lib()
    st, raw, img = _build([(0, 144, 160), (2, 256, 160)])
    assert st == 0
    words = np.frombuffer(C.string_at(img, 32), dtype=np.int32)
    assert words[1:4].tolist() == [2, 4, 2]                                      # n_mats, n_ranges, n_classes
    tail = np.frombuffer(C.string_at(img + 32 + 2 * 64 + 2 * 64, 16), dtype=np.int32)
    assert tail.tolist() == [0, -1, 1, -1]                                       # range -> matrix
    assert _build([])[0] == 0
    assert _build([(0, 144, 161)], ranges=None)[0] == 0                          # without the ranges the element count is not checked
    assert _build([(0, 144, 161)])[0] == BAD_ARG and "23040 elements" in _err()
    assert _build([(1, 1, 7)])[0] == 0                                           # no lower limit: the caller's selection keeps the small ones away
    assert _build([(0, 2049, 2050)], ranges=None)[0] == BAD_ARG and "above 2048" in _err()
    assert _build([(0, 2048, 4096)], ranges=None)[0] == 0
    assert _build([(0, 144, 160), (0, 160, 144)])[0] == BAD_ARG and "twice" in _err()
    assert _build([(0, 144, 160)], small=[(1, 1, 7), (0, 144, 160)])[0] == BAD_ARG and "twice" in _err() and "small list" in _err()
    assert _build([(0, 144, 160)], small=[(1, 1, 7)])[0] == 0
    assert _build([(4, 144, 160)])[0] == BAD_ARG and _build([(-1, 144, 160)])[0] == BAD_ARG
    assert _build([(1, 0, 7)])[0] == BAD_ARG and _build([(1, 7, -1)])[0] == BAD_ARG
    assert _build([(0, 144, 160)], mats=None)[0] == BAD_ARG and _build([(0, 144, 160)], image=None)[0] == BAD_ARG
    assert _build([(0, 144, 160)], n_ranges=-1)[0] == BAD_ARG
    assert _build([(0, 144, 160)], nbytes=64)[0] == WORKSPACE
    # the small entry point keeps refusing a short side above 128, with its present message
    raw2, img2 = _buf(4096)
    assert L.avmoe_opt_muon_table_build(None, 4, _mats([(3, 129, 130)]), 1, img2, 4096) == BAD_ARG
    assert _err() == "avmoe_opt_muon_table_build: matrix 0 is 129 x 130: its short side is above 128"


def test_the_classes_and_the_size_function():
    """two 144 x 160 and one 160 x 144 are one class after orientation, 256 x 160 another; the workspace holds the constant vectors, the
    block sums, two staging buffers and A and B per class, and the slabs of a split Gram product"""
    L = _capi.lib()
    rows = [(0, 144, 160), (1, 256, 160), (2, 160, 144), (3, 144, 160)]
    lay = cm.OptMuonLargeLayout()
    total = L.avmoe_opt_muon_large_bytes(5, _mats(rows), 4, C.byref(lay))
    assert total == lay.table_bytes + lay.workspace_bytes + lay.report_bytes and lay.n_classes == 2
    assert lay.table_bytes % 16 == 0 and lay.workspace_bytes % 16 == 0 and lay.report_bytes % 16 == 0
    assert 32 + 4 * 64 + 2 * 64 + 5 * 4 <= lay.table_bytes < 32 + 4 * 64 + 2 * 64 + 5 * 4 + 16
    assert lay.report_bytes == 16 + 16
    blocks = 3 * 23 + 40                                                         # 1024-element blocks of the four matrices
    want = 2 * 2048 * 4 + 8 * blocks + 4 * (3 * (2 * 144 * 160 + 2 * 144 * 144) + (2 * 160 * 256 + 2 * 160 * 160))
    assert want <= lay.workspace_bytes < want + 32
    raw, img = _buf(int(lay.table_bytes))
    assert L.avmoe_opt_muon_large_table_build(None, 5, _mats(rows), 4, None, 0, img, int(lay.table_bytes)) == 0
    cls, of = (cm.OptMuonClass * 4)(), (C.c_int32 * 4)()
    assert L.avmoe_opt_muon_large_classes(img, cls, 4, of) == 2
    assert [(c.d, c.L, c.count, c.ksplit) for c in cls[:2]] == [(144, 160, 3, 1), (160, 256, 1, 1)] and list(of) == [0, 1, 0, 0]
    assert L.avmoe_opt_muon_large_classes(img, None, 0, None) == 2
    zero = C.create_string_buffer(64)
    assert L.avmoe_opt_muon_large_classes(zero, None, 0, None) == BAD_ARG and L.avmoe_opt_muon_large_classes(None, None, 0, None) == BAD_ARG
    # padding to the engine's 16-byte rows: 129 x 130 stages as 132 x 132; a long thin matrix splits the Gram product's K
    lay2 = cm.OptMuonLargeLayout()
    assert L.avmoe_opt_muon_large_bytes(2, _mats([(0, 129, 130), (1, 128, 4096)]), 2, C.byref(lay2)) > 0 and lay2.n_classes == 2
    want2 = 2 * 2048 * 4 + 8 * (17 + 512) + 4 * (2 * 132 * 132 + 2 * 129 * 132) + 4 * (2 * 128 * 4096 + 2 * 128 * 128 + 8 * 128 * 128)
    assert want2 <= lay2.workspace_bytes < want2 + 32
    for bad in ((-1, 0), (1, -1), (1, 2)):
        lay2.table_bytes = 7
        assert L.avmoe_opt_muon_large_bytes(bad[0], _mats([(0, 144, 160), (0, 144, 160)]), bad[1], C.byref(lay2)) == 0 and lay2.table_bytes == 7
        assert "avmoe_opt_muon_large_bytes" in _err()
    assert L.avmoe_opt_muon_large_bytes(2, _mats([(0, 2049, 2049)]), 1, None) == 0 and "above 2048" in _err()


def _calls():
    L = _capi.lib()
    raw, base = _buf(32768)
    table, state, shadows, hold, mats, work, ws, report, large, lws, lreport = (base + 2048 * k for k in range(11))
    lay = cm.OptMuonLargeLayout()
    rows = _mats([(0, 144, 160)])
    assert L.avmoe_opt_muon_large_bytes(2, rows, 1, C.byref(lay)) > 0
    hraw, host = _buf(int(lay.table_bytes))
    assert L.avmoe_opt_muon_large_table_build(None, 2, rows, 1, None, 0, host, int(lay.table_bytes)) == 0
    defaults = dict(momentum=0.95, nesterov=1, ns_steps=5, scale=0)

    def step(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold,
             mats=mats, n_mats=1, work=work, ws=ws, report=report, large=large, large_host=host, n_large=1, lws=lws, lreport=lreport, **c):
        cs = cm.OptMuon(**{**defaults, **c})
        return L.avmoe_opt_muon_step_large(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows, hold, mats, n_mats, work,
                                           C.byref(cs), ws, report, large, large_host, n_large, lws, lreport)

    def small(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold,
              mats=mats, n_mats=1, work=work, ws=ws, report=report, **c):
        cs = cm.OptMuon(**{**defaults, **c})
        return L.avmoe_opt_muon_step(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows, hold, mats, n_mats, work, C.byref(cs),
                                     ws, report)

    def ns(large=large, large_host=host, n_large=1, work=work, ns_steps=5, lws=lws):
        return L.avmoe_opt_muon_ns_large(large, large_host, n_large, work, ns_steps, lws, None)

    ptrs = dict(table=table, state=state, shadows=shadows, hold=hold, mats=mats, work=work, ws=ws, report=report, large=large, lws=lws, lreport=lreport,
                host=host)
    return (raw, hraw), ptrs, step, small, ns


def test_the_step_refuses_what_avmoe_opt_muon_step_refuses():
    from tests.test_flat_adam_lamb_api import REFUSALS, _resolve
    keep, ptrs, step, small, ns = _calls()
    own = [dict(mats=None), dict(work=None), dict(ws=None), dict(report=None), dict(n_mats=-1), dict(ns_steps=0), dict(ns_steps=17),
           dict(momentum=1.0), dict(nesterov=2), dict(scale=2), dict(mats=8), dict(work=4), dict(ws=4), dict(report=8)]
    for hold in (ptrs["hold"], None):
        for kw in REFUSALS + own:
            kw = _resolve(kw, ptrs)
            want = small(hold=hold, **kw)
            assert want in (BAD_ARG, ALIGNMENT), kw
            msg = _err().replace("avmoe_opt_muon_step", "")
            assert step(hold=hold, **kw) == want and _err().replace("avmoe_opt_muon_step_large", "") == msg, kw


def test_the_launching_calls_refuse_their_own_arguments_before_any_launch():
    keep, ptrs, step, small, ns = _calls()
    for hold in (ptrs["hold"], None):
        for name in ("large", "large_host", "lws", "lreport"):
            assert step(hold=hold, **{name: None}) == BAD_ARG and "NULL" in _err(), name
        assert step(hold=hold, n_large=-1) == BAD_ARG
        assert step(hold=hold, n_large=2) == BAD_ARG and "host copy" in _err()             # the host image says one matrix
        assert step(hold=hold, n_ranges=3) == BAD_ARG and "host copy" in _err()            # ... and two ranges
        assert step(hold=hold, large_host=ptrs["lws"]) == BAD_ARG and "host copy" in _err()      # zeros are no image
        assert step(hold=hold, large=ptrs["large"] + 8) == ALIGNMENT and "large image" in _err()
        assert step(hold=hold, lws=ptrs["lws"] + 8) == ALIGNMENT and "large workspace" in _err()
        assert step(hold=hold, lreport=ptrs["lreport"] + 8) == ALIGNMENT and "large report" in _err()
        assert step(hold=hold, large=None, lws=ptrs["lws"] + 8) == BAD_ARG                 # NULL comes before alignment
    assert ns(large=None) == BAD_ARG and ns(large_host=None) == BAD_ARG and ns(work=None) == BAD_ARG and ns(lws=None) == BAD_ARG
    assert ns(n_large=-1) == BAD_ARG and ns(n_large=2) == BAD_ARG
    assert ns(ns_steps=0) == BAD_ARG and ns(ns_steps=17) == BAD_ARG and "1..16" in _err()
    assert ns(large=ptrs["large"] + 4) == ALIGNMENT and ns(work=ptrs["work"] + 4) == ALIGNMENT and ns(lws=ptrs["lws"] + 4) == ALIGNMENT
    # nothing to launch: an empty list
    L = _capi.lib()
    lay = cm.OptMuonLargeLayout()
    assert L.avmoe_opt_muon_large_bytes(2, None, 0, C.byref(lay)) > 0 and lay.n_classes == 0
    raw, empty = _buf(int(lay.table_bytes))
    assert L.avmoe_opt_muon_large_table_build(None, 2, None, 0, None, 0, empty, int(lay.table_bytes)) == 0
    assert ns(large_host=empty, n_large=0) == 0
    assert step(large_host=empty, n_large=0, n_ranges=0, n_blocks=0, n_mats=0, shadows=None) == BAD_ARG      # the image says two ranges
    raw0, empty0 = _buf(int(lay.table_bytes))
    assert L.avmoe_opt_muon_large_table_build(None, 0, None, 0, None, 0, empty0, int(lay.table_bytes)) == 0
    assert step(large_host=empty0, n_large=0, n_ranges=0, n_blocks=0, n_mats=0, shadows=None) == 0


def _ns32_chunked(G, steps=5, chunk=64):
    """the iteration in numpy fp32 with every product summed in chunks of its contraction index (another order of the same fp32 sums)"""
    a, b, c = (np.float32(v) for v in R.NS_COEFFS)
    G = np.asarray(G, dtype=np.float32)
    nrm = np.sqrt(np.sum(G.astype(np.float64) ** 2))
    X = (G.astype(np.float64) / (nrm + R.NS_EPS)).astype(np.float32)
    tall = G.shape[0] > G.shape[1]
    if tall:
        X = X.T

    def mm(p, q):
        out = np.zeros((p.shape[0], q.shape[1]), dtype=np.float32)
        for k in range(0, p.shape[1], chunk):
            out += p[:, k:k + chunk] @ q[k:k + chunk]
        return out
    for _ in range(steps):
        A = mm(X, X.T)
        B = b * A + c * mm(A, A)
        X = a * X + mm(B, X)
    return np.ascontiguousarray(X.T if tall else X)


@pytest.mark.parametrize("shape", NS_SHAPES, ids=["x".join(str(v) for v in s) for s in NS_SHAPES])
def test_the_fp32_restatement_stays_inside_the_device_tests_bound(shape):
    """numpy fp32 in two summation orders against fp64 on every input of tests/test_flat_adam_muon_large_gpu.py's sub-op test: both stay
    inside NS_FACTOR yardsticks, so on the device the bound can only be broken by the kernel"""
    rows, cols = FlatAdam.muon_large_shape_of(torch.empty(shape))
    rng = np.random.default_rng(rows * 10007 + cols + len(shape))
    assert 1.0 < NS_FACTOR <= 8.0
    for kind in KINDS:
        x = R.inputs(kind, rows, cols, rng)
        o64, tol = R.ns_tolerance(x, 5, NS_FACTOR)
        for name, o32 in (("plain", R.ns(x, 5, np.float32)), ("chunked", _ns32_chunked(x))):
            err = float(np.max(np.abs(o32.astype(np.float64) - o64))) if o64.size else 0.0
            assert np.isfinite(o32).all() and err <= tol, (kind, name, err, tol)
        if kind == "zeros":
            assert not o64.any() and tol == 0.0
