"""Host side of orthogonalised momentum in FlatAdam (include/avmoe.h: avmoe_opt_muon_bytes, avmoe_opt_muon_table_build,
avmoe_opt_muon_step, avmoe_opt_muon_ns; avmoe_amd.train.FlatAdam(muon=...)): the symbols and layouts the binding relies on, the size
function, the checks of the image builder and of the two launching calls (they precede any launch: host pointers and a NULL stream are
enough, no GPU is needed), every ValueError of the constructor, and the selection rule on a MoEAdapter of each variant."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd import adapters
from avmoe_amd.train import FlatAdam
from tests import muon_ref
from tests.golden_util import load_golden
from tests.test_adapters_api import _opt
from tests.test_flat_adam_lamb_api import _buf, _err, _reducer, BAD_ARG, ALIGNMENT

WORKSPACE = -4


def test_header_declares_and_library_exports_the_entry_points():
    L = _capi.lib()
    header = open(_capi.HEADER_PATH).read()
    for name in ("avmoe_opt_muon_bytes", "avmoe_opt_muon_table_build", "avmoe_opt_muon_step", "avmoe_opt_muon_ns"):
        assert name in _capi.exported_symbols() and hasattr(L, name) and name in header, name
    assert L.avmoe_abi_version() == 11
    for struct in ("avmoe_opt_muon_mat", "avmoe_opt_muon", "avmoe_opt_muon_layout"):
        assert f"typedef struct {struct} " in header, struct
    assert C.sizeof(cm.OptMuonMat) == 16 and C.sizeof(cm.OptMuon) == 16 and C.sizeof(cm.OptMuonLayout) == 3 * C.sizeof(C.c_size_t)
    assert "#define AVMOE_MUON_MAX_DIM 128" in header and FlatAdam.MUON_MAX_DIM == 128
    assert C.sizeof(cm.OptRange) == 48 and cm.OPT_STATE_BYTES == 64          # no flag, no new word: range and state block are what they were


def test_the_size_function_on_good_and_bad_counts():
    L = _capi.lib()
    lay = cm.OptMuonLayout()
    for n_ranges, n_blocks, n_mats in ((0, 0, 0), (1, 1, 1), (13, 80, 7), (466, 4000, 300), (5, 0, 0)):
        total = L.avmoe_opt_muon_bytes(n_ranges, n_blocks, n_mats, C.byref(lay))
        assert lay.table_bytes % 16 == 0 and lay.workspace_bytes % 16 == 0 and lay.report_bytes % 16 == 0
        assert 16 + 16 * n_mats + 4 * n_ranges <= lay.table_bytes < 16 + 16 * n_mats + 4 * n_ranges + 16
        assert 8 * max(n_blocks, 1) <= lay.workspace_bytes < 8 * max(n_blocks, 1) + 16          # one double per table block
        assert 16 + 4 * max(n_mats, 1) <= lay.report_bytes < 16 + 4 * max(n_mats, 1) + 16       # header + one float per matrix
        assert total == lay.table_bytes + lay.workspace_bytes + lay.report_bytes
    lay.table_bytes = 7
    for bad in ((-1, 0, 0), (0, -1, 0), (3, 1, -1), (3, 1, 4), (1, 1 << 31, 1)):
        assert L.avmoe_opt_muon_bytes(*bad, C.byref(lay)) == 0 and "avmoe_opt_muon_bytes" in _err(), bad
    assert lay.table_bytes == 7


def _ranges(ns):
    arr = (cm.OptRange * len(ns))()
    for r, n in zip(arr, ns):
        r.param = r.grad = r.exp_avg = r.exp_avg_sq = 64
        r.n = n
    return arr


def _mats(rows):
    arr = (cm.OptMuonMat * max(1, len(rows)))()
    for m, (rg, r, c) in zip(arr, rows):
        m.range, m.rows, m.cols = rg, r, c
    return arr


def test_the_image_builder_checks_the_matrices_on_the_host():
    L = _capi.lib()
    raw, img = _buf(4096)
    ranges = _ranges([128, 7, 600, 129 * 130])

    def build(rows, ranges=ranges, n_ranges=4, image=img, nbytes=4096, mats="own"):
        return L.avmoe_opt_muon_table_build(ranges, n_ranges, _mats(rows) if mats == "own" else mats, len(rows), image, nbytes)

    assert build([(0, 4, 32), (2, 200, 3)]) == 0
    words = np.frombuffer(C.string_at(img, 16 + 2 * 16 + 4 * 4), dtype=np.int32)
    assert words[1] == 2 and words[2] == 4                                      # n_mats, n_ranges
    assert words[4:12].tolist() == [0, 4, 32, 0, 2, 200, 3, 0]                  # the matrices, in the caller's order
    assert words[12:16].tolist() == [0, -1, 1, -1]                              # range -> matrix
    assert build([]) == 0
    assert build([(0, 4, 32)], ranges=None) == 0                                # without the ranges the element count is not checked
    assert build([(0, 4, 31)], ranges=None) == 0
    assert build([(0, 4, 31)]) == BAD_ARG and "128 elements" in _err()           # rows * cols != n of the range
    assert build([(3, 129, 130)]) == BAD_ARG and "above 128" in _err()           # min(rows, cols) > 128
    assert build([(0, 4, 32), (0, 32, 4)]) == BAD_ARG and "twice" in _err()      # a range named twice
    assert build([(4, 4, 32)]) == BAD_ARG and build([(-1, 4, 32)]) == BAD_ARG    # a range outside the table
    assert build([(1, 0, 7)]) == BAD_ARG and build([(1, 7, -1)]) == BAD_ARG
    assert build([(0, 4, 32)], mats=None) == BAD_ARG and build([(0, 4, 32)], image=None) == BAD_ARG
    assert build([(0, 4, 32)], n_ranges=-1) == BAD_ARG
    assert build([(0, 4, 32)], nbytes=32) == WORKSPACE


def _calls():
    L = _capi.lib()
    raw, base = _buf(20480)
    table, state, shadows, hold, mats, work, ws, report = (base + 2048 * k for k in range(8))
    defaults = dict(momentum=0.95, nesterov=1, ns_steps=5, scale=0)

    def step(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold,
             mats=mats, n_mats=1, work=work, ws=ws, report=report, consts="own", **c):
        cs = cm.OptMuon(**{**defaults, **c})
        return L.avmoe_opt_muon_step(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows, hold, mats, n_mats, work,
                                     C.byref(cs) if consts == "own" else consts, ws, report)

    def sam(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold):
        return L.avmoe_opt_adam_step_sam(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows, hold)

    def ema(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2):
        return L.avmoe_opt_adam_step_ema(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows)

    def ns(mats=mats, n_mats=1, work=work, ns_steps=5):
        return L.avmoe_opt_muon_ns(mats, n_mats, work, ns_steps, None)

    return raw, dict(table=table, state=state, shadows=shadows, hold=hold, mats=mats, work=work, ws=ws, report=report), step, sam, ema, ns


def test_the_step_refuses_what_the_update_entry_points_refuse():
    from tests.test_flat_adam_lamb_api import REFUSALS, _resolve
    raw, ptrs, step, sam, ema, ns = _calls()
    for kw in REFUSALS:
        kw = _resolve(kw, ptrs)
        want = sam(**kw)
        assert want in (BAD_ARG, ALIGNMENT), kw
        msg = _err().replace("avmoe_opt_adam_step_sam", "")
        assert step(**kw) == want and _err().replace("avmoe_opt_muon_step", "") == msg, kw
        want = ema(**kw)
        msg = _err().replace("avmoe_opt_adam_step_ema", "")
        assert step(hold=None, **kw) == want and _err().replace("avmoe_opt_muon_step", "") == msg, kw


def test_the_launching_calls_refuse_their_own_arguments_before_any_launch():
    raw, ptrs, step, sam, ema, ns = _calls()
    for hold in (ptrs["hold"], None):
        for name in ("mats", "work", "ws", "report", "consts"):
            assert step(hold=hold, **{name: None}) == BAD_ARG and "NULL" in _err(), name
        assert step(hold=hold, n_mats=-1) == BAD_ARG
        for bad in (dict(ns_steps=0), dict(ns_steps=17), dict(ns_steps=-1), dict(momentum=1.0), dict(momentum=-0.1), dict(momentum=float("nan")),
                    dict(nesterov=2), dict(scale=2), dict(scale=-1)):
            assert step(hold=hold, **bad) == BAD_ARG, bad
        assert step(hold=hold, mats=ptrs["mats"] + 8) == ALIGNMENT and "image" in _err()
        assert step(hold=hold, work=ptrs["work"] + 4) == ALIGNMENT and "work" in _err()
        assert step(hold=hold, ws=ptrs["ws"] + 4) == ALIGNMENT and "workspace" in _err()
        assert step(hold=hold, report=ptrs["report"] + 8) == ALIGNMENT and "report" in _err()
        assert step(hold=hold, mats=None, report=ptrs["report"] + 8) == BAD_ARG            # NULL comes before alignment
        assert step(hold=hold, n_ranges=0, n_blocks=0, n_mats=0, shadows=None) == 0        # nothing to launch
    assert ns(mats=None) == BAD_ARG and ns(work=None) == BAD_ARG and ns(n_mats=-1) == BAD_ARG
    assert ns(ns_steps=0) == BAD_ARG and ns(ns_steps=17) == BAD_ARG and "1..16" in _err()
    assert ns(mats=ptrs["mats"] + 4) == ALIGNMENT and ns(work=ptrs["work"] + 4) == ALIGNMENT
    assert ns(n_mats=0) == 0


BAD_CTOR = [dict(muon=1), dict(muon=None), dict(muon="yes"),
            dict(muon=True, muon_momentum=1.0), dict(muon=True, muon_momentum=-0.1), dict(muon=True, muon_momentum=float("nan")),
            dict(muon=True, muon_momentum=1.0 - 1e-9), dict(muon=True, muon_nesterov=1), dict(muon=True, muon_nesterov=None),
            dict(muon=True, muon_ns_steps=0), dict(muon=True, muon_ns_steps=17), dict(muon=True, muon_ns_steps=5.0), dict(muon=True, muon_ns_steps=True),
            dict(muon=True, muon_scale="rms"), dict(muon=True, muon_scale=None), dict(muon=True, muon_max_numel=0), dict(muon=True, muon_max_numel=1e5),
            dict(muon_momentum=0.9), dict(muon_nesterov=False), dict(muon_ns_steps=3), dict(muon_scale="original"), dict(muon_max_numel=1000),
            dict(muon=False, muon_momentum=0.9),
            dict(muon=True, trust_ratio=True), dict(muon=True, prodigy=True)]


@pytest.mark.parametrize("kw", BAD_CTOR, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD_CTOR])
def test_bad_constructor_arguments_raise_value_error_before_anything_is_touched(kw):
    red, w, b = _reducer()
    ptrs = (w.data_ptr(), b.data_ptr())
    with pytest.raises(ValueError, match="muon"):
        FlatAdam(red, **kw)
    assert (w.data_ptr(), b.data_ptr()) == ptrs


@pytest.mark.parametrize("value", [1, 0, None, "no", 1.0])
def test_a_groups_muon_must_be_a_bool(value):
    red, w, b = _reducer()
    ptrs = (w.data_ptr(), b.data_ptr())
    with pytest.raises(ValueError, match="muon"):
        FlatAdam(red, muon=True, param_groups=[{"params": [w], "muon": value}])
    assert (w.data_ptr(), b.data_ptr()) == ptrs


def test_true_on_a_parameter_that_does_not_fit_names_it():
    red, w, b = _reducer()
    ptrs = (w.data_ptr(), b.data_ptr())
    with pytest.raises(ValueError, match=r"parameter 1 of shape \(7,\)"):
        FlatAdam(red, muon=True, param_groups=[{"params": [w, b], "muon": True}])
    with pytest.raises(ValueError, match=r"parameter 0 of shape \(3, 4\).*muon_max_numel = 11"):
        FlatAdam(red, muon=True, muon_max_numel=11, param_groups=[{"params": [w], "muon": True}])
    assert (w.data_ptr(), b.data_ptr()) == ptrs


def test_muon_selects_the_device_path_and_the_defaults():
    red, w, b = _reducer()
    with pytest.raises(_capi.AvmoeError):                    # a good value gets as far as the buckets: the device path has no CPU fallback
        FlatAdam(red, muon=True, param_groups=[{"params": [w], "muon": False}])
    sig = inspect.signature(FlatAdam.__init__).parameters
    assert [sig[k].default for k in ("muon", "muon_momentum", "muon_nesterov", "muon_ns_steps", "muon_scale", "muon_max_numel")] == \
        [False, 0.95, True, 5, "match_rms_adamw", 262144]
    assert "Orthogonalised momentum" in FlatAdam.__doc__ and "verified on one rank" in FlatAdam.__doc__
    assert FlatAdam._check_muon(True, 0.9, False, 3, "original", 100) == (True, float(np.float32(0.9)), False, 3, "original", 100)
    for name in ("orthogonalized", "muon_scales", "last_muon_updates", "last_muon_norms", "muon_shape_of", "muon_select", "muon_scale_of"):
        assert hasattr(FlatAdam, name), name


def test_muon_shape_of_and_the_scales():
    z = torch.zeros
    f = FlatAdam.muon_shape_of
    assert f(z(64, 24, 1, 1)) == (64, 24)                    # a conv weight, flattened as torch.optim.Muon's users do
    assert f(z(12, 48, 3, 3)) == (12, 432) and f(z(87, 768)) == (87, 768) and f(z(768, 32)) == (768, 32) and f(z(1, 5)) == (1, 5)
    assert f(z(128, 2048)) == (128, 2048) and f(z(128, 2049)) is None                   # numel <= 262144
    assert f(z(129, 129)) is None and f(z(128, 128)) == (128, 128) and f(z(129, 128)) == (129, 128)      # the SHORT side <= 128
    assert f(z(7)) is None and f(z(())) is None and f(z(0, 4)) is None
    assert f(z(64, 24), max_numel=1535) is None and f(z(64, 24), max_numel=1536) == (64, 24)
    g = FlatAdam.muon_scale_of
    for rows, cols in ((64, 24), (4, 32), (768, 32), (87, 200), (16, 16)):
        assert g(rows, cols) == float(np.float32(0.2 * math.sqrt(max(rows, cols)))) == g(rows, cols, "match_rms_adamw")
        assert g(rows, cols, "original") == float(np.float32(math.sqrt(max(1.0, rows / cols))))
        assert abs(g(rows, cols) - muon_ref.scale_of(rows, cols)) <= 1e-7 * g(rows, cols)
        assert abs(g(rows, cols, "original") - muon_ref.scale_of(rows, cols, "original")) <= 1e-7 * g(rows, cols, "original")
    assert g(4, 32, "original") == 1.0 and g(768, 32, "original") == float(np.float32(math.sqrt(24.0)))


ORTHOGONALIZED_SUFFIXES = ("down_sampler.weight", "up_sampler.weight", "my_tokens", "router.0.weight", "router.2.weight", "router.4.weight",
                           "conv_adapter.weight", "fc.weight")


def small_site():
    """the ave_train fixture's configuration: every matrix of it fits"""
    _, cfg, _ = load_golden("ave_train")
    m = adapters.MoEAdapter(input_dim=cfg.Cx, output_dim=cfg.Cx, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=_opt(cfg),
                            conv_dim_in=cfg.Ny, conv_dim_out=cfg.Nx, linear_in=cfg.Cy, linear_out=cfg.Cx, reduction_factor=cfg.reduction,
                            use_bn=cfg.use_bn, use_gate=cfg.use_gate, num_tk=cfg.K)
    return m


def small_site_orthogonalized(m):
    """name -> whether `muon=True` orthogonalises it, at the small site: every hidden matrix, and nothing else"""
    return {n: n.endswith(ORTHOGONALIZED_SUFFIXES) for n, _ in m.named_parameters()}


def test_the_selection_at_the_small_site():
    m = small_site()
    names = [n for n, _ in m.named_parameters()]
    sel = FlatAdam.muon_select([p for _, p in m.named_parameters()])
    want = small_site_orthogonalized(m)
    assert [s is not None for s in sel] == [want[n] for n in names]
    assert sum(want.values()) >= 13 and not any(want[n] for n in names if "gate" in n or ".bn" in n or ".ln_" in n or n.endswith("bias"))


VARIANTS = {"ave": (adapters.MoEAdapter, dict(reduction_factor=8, use_bn=True, use_gate=True, num_tk=87)),
            "avs": (adapters.MoEAdapterAVS, dict(reduction_factor=8, use_bn=True, use_gate=True, num_tk=87)),
            "avqa": (adapters.MoEAdapterAVQA, dict(reduction_factor=8, use_bn=True, use_gate=True)),
            "avvp": (adapters.MoEAdapterAVVP, {})}


@pytest.mark.parametrize("which", list(VARIANTS))
def test_the_selection_rule_on_each_variant(which):
    """C = 256 with 144 x 160 tokens and a 160-wide other modality: the experts' samplers, the latent tokens and the router's layers are
    orthogonalised; conv_adapter (144 x 160) and fc (256 x 160) have a short side above 128 and take Adam, like gates, norms and biases"""
    _, cfg, _ = load_golden("ave_train")
    cls, kw = VARIANTS[which]
    m = cls(input_dim=256, output_dim=256, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=_opt(cfg), conv_dim_in=160, conv_dim_out=144,
            linear_in=160, linear_out=256, **kw)
    named = list(m.named_parameters())
    sel = dict(zip((n for n, _ in named), FlatAdam.muon_select([p for _, p in named])))
    on = sorted({n.split("experts.")[-1].split(".", 1)[-1] if "experts." in n else n for n, s in sel.items() if s is not None})
    print(which, on)
    assert on == sorted(["down_sampler.weight", "up_sampler.weight", "my_tokens", "router.0.weight", "router.2.weight", "router.4.weight"])
    assert sel["conv_adapter.weight"] is None and sel["fc.weight"] is None
    assert tuple(dict(named)["conv_adapter.weight"].shape[:2]) == (144, 160) and tuple(dict(named)["fc.weight"].shape) == (256, 160)
    assert sel["router.0.weight"] == (128, 512) and sel["router.4.weight"] == (4, 32)
    for n, s in sel.items():
        if "gate" in n or ".bn" in n or ".ln_" in n or n.endswith("bias"):
            assert s is None, n
    ds = next(n for n in sel if n.endswith("down_sampler.weight"))
    assert dict(named)[ds].dim() == 4 and sel[ds] == (dict(named)[ds].shape[0], dict(named)[ds][0].numel())
    # router.0 is orthogonalised only where it fits the numel limit; a group switches a matrix off, and True on conv_adapter raises
    params = [p for _, p in named]
    small = dict(zip((n for n, _ in named), FlatAdam.muon_select(params, muon_max_numel=65535)))
    assert small["router.0.weight"] is None and small["router.2.weight"] == (32, 128)
    off = dict(zip((n for n, _ in named), FlatAdam.muon_select(params, [{"params": [dict(named)["router.2.weight"]], "muon": False}])))
    assert off["router.2.weight"] is None and off["router.4.weight"] == (4, 32)
    with pytest.raises(ValueError, match=r"shape \(144, 160, 1, 1\)"):
        FlatAdam.muon_select(params, [{"params": [dict(named)["conv_adapter.weight"]], "muon": True}])
