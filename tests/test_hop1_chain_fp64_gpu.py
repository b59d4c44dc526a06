"""The hop-1 chain BETWEEN its two ends on Y -- every intermediate of moe_forward.cpp:92-180 and of the backward's phases 5 / 6a
(moe_backward.cpp:248-331, :336-464) that tests/test_stream_products_gpu.py does not reach -- link by link against fp64 of the link's own
operands as stored in the workspace (tests/hop1_ref.py: references, bounds, input families; tests/test_hop1_checker.py shows on the CPU what
such a check catches).  One site per (shape, dtype, family), one Recorder per site: a run reports every failing link.

The forward runs whole and L1 / TV are read from scratch behind it (no two named buffers share memory); the backward runs in sections 1, 32, 8
(avmoe_moe_backward_part) and is read after 32 (dTW, dTT, k_finish_dT) and after 8 (everything else).  Every site runs twice: the checked
buffers hold the same bytes; guard bands and the NaN poison of L1's padding are intact.  Each link is counted under the kernel family the profiler saw; the four per-frame products (L1, [Bm | ab], dA1,
dR^T) must be on `gemm_frames` exactly where launch_gemm_frames serves them (hop1_ref.frames_serves transcribes frame_gemm.hip:336-350; the
profiler has ONE name for the plain, the long (K > 256) and the transposed form, so the form is the one that follows from the shape, and the
number of `gemm_frames` scopes is asserted), and where a form steps aside the test says why.

fp32 sites (pad_77_71 and the AVS v2 site) run the engine's three-plane and, for dWf / dWcK, two-plane form; their stores are fp32.  The AVS
v2 site runs its backward whole and is held through what survives it (test_hop1_chain_of_the_v2_site).  See DESIGN_CURRENT.md, "What guards
the hop-1 chain".
"""
import ctypes as C
import os

import pytest
import torch

from oracle import avmoe_oracle as O
from tests import hop1_ref as H

pytestmark = pytest.mark.gpu

# (frames, N, M, E_m, E_s) at C = Cy = 768, 2 groups, reduction 12, K = 32
SHAPES = {
    "pad_77_71": (32, 77, 71, 2, 2),          # N % 4 = 1, Np = 80; M % 4 = 3, Mb = 72 != Mk = 80; all four per-frame products on gemm_frames; 65 rows per frame as the tall matrix
    "one_cross_66": (33, 196, 66, 1, 3),      # Kcyb = 33, odd frame count, M % 4 = 2
    "long_k_y": (33, 200, 300, 2, 2),         # L1 / dA1 with K > 256: kk_frame_gemm_long, last block a single frame
    "long_k_x": (32, 300, 100, 2, 2),         # Bm / dRT long; dRT the transposed instantiation
    "short_20": (34, 20, 65, 2, 2),           # N < 64: L1 / dA1 step aside; Bm / dRT on gemm_frames with K = 20; M % 4 = 1
    "rows_1100": (2, 1100, 64, 2, 2),         # _reg<16> in both softmax directions
    "rows_4100": (2, 4100, 40, 2, 2),         # the plain kernels (n, ld > 4096)
}
RAGGED = {"pad_77_71", "one_cross_66", "short_20", "rows_1100", "rows_4100", "v2_k20"}      # N or M no multiple of 8 / of the 4-vectors
FAMILY_SHAPES = ("pad_77_71", "one_cross_66", "rows_1100")                        # flat and peaked beside the default draw
CASES = [(s, "default", "bf16") for s in SHAPES] + [(s, f, "bf16") for s in FAMILY_SHAPES for f in ("flat", "peaked")] + [("pad_77_71", "default", "fp32")]
CHECKED = {}      # link -> {(shape, family, dtype): (kernel family seen, worst err / bound)}
TEXTS = set()     # kernel texts / forms seen by name or by the shape that selects them

FWD_BUFS = ("WcK", "WcT", "WfT", "rw", "wbar", "T0T", "Qx", "qrqb", "Rext", "A1y", "BmX", "V", "Text", "Tsum", "TT", "TW", "rin", "TV")
BWD_BUFS = ("dTW", "dTT", "dTy", "dabx", "dV", "dBm", "dBmT", "dvec", "L1", "dL1", "dRT", "dWcK", "dqp", "dT0", "dQT", "dWf")


def _cfg(N, M, E_m, E_s):
    return O.AdapterConfig(Cx=768, Nx=N, Cy=768, Ny=M, reduction=12, groups=2, K=32, E_m=E_m, E_s=E_s, variant="ave")


class Site:
    """One training-mode site on cuda:0 (tests/moe_gpu_util.py::MoeRun: NaN-poisoned workspaces, guard bands) with the parameters of one
    input family, the backward in sections and every hop-1 buffer as a typed device view."""

    def __init__(self, cfg, S, family, bf16=True, seed=21):
        from tests.moe_gpu_util import MoeRun
        P, Bf = O.init_params(cfg, seed=seed)
        P = H.apply_family(P, family, cfg)
        g = torch.Generator().manual_seed(seed + 100)
        X = H.family_X(0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g), family, cfg)
        Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
        self.G = torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
        self.cfg, self.S = cfg, S
        self.run = MoeRun(cfg, P, Bf, X, Y, bf16=bf16, training=True)
        self.d = H.Dims(cfg, S, bf16, {k: v[2] for k, v in self.run.table.items()})

    def view(self, name):
        kind, shape = self.d.shapes()[name]
        region, off, nbytes = self.run.table[name]
        raw = (self.run.saved if region == 0 else self.run.scratch)[off:off + nbytes]
        n = 1
        for k in shape:
            n *= k
        return raw.view(torch.float32 if kind == "f" else self.d.T)[:n].reshape(shape)

    def bufs(self):
        B = {k: self.view(k) for k in self.d.shapes()}
        B.update(self.run.params)
        B["Y"], B["X"] = self.run.Y, self.run.X
        B["grads"], B["grads_tail"] = getattr(self.run, "grads", None), getattr(self, "tails", None)
        return B

    def raw(self, names):
        out = {}
        for k in names:
            region, off, nbytes = self.run.table[k]
            out[k] = (self.run.saved if region == 0 else self.run.scratch)[off:off + nbytes].clone()
        return out

    def begin_backward(self):
        r = self.run
        from avmoe_amd import _capi_moe as cm
        r.dOut = self.G.to(r.dev, r.tdt).contiguous()
        r.dX = torch.full_like(r.X, float("nan"))
        r.dY = torch.full_like(r.Y, float("nan"))
        r.grads = {k: torch.full_like(v, float("nan")) for k, v in r.params.items()}
        # the my_tokens gradients lie in front of NaN rows of the same allocation: a row k >= K written shows there (hop1_ref.link_finalize)
        self.tails = {}
        for k in self.d.tok_keys:
            K = self.cfg.K
            big = torch.full((K + max(self.d.Kp - K, 1), self.cfg.Cx), float("nan"), device=r.dev)
            r.grads[k], self.tails[k] = big[:K], big[K:]
        r.gptrs = cm.make_ptrs(r.grads, self.cfg.E_m, self.cfg.E_s)
        r.lbw = torch.zeros(1, device=r.dev, dtype=torch.float32)

    def part(self, parts):
        from avmoe_amd import _capi as capi
        r = self.run
        st = r.L.avmoe_moe_backward_part(C.byref(r.desc), r.X.data_ptr(), r.Y.data_ptr(), C.byref(r.ptrs), r.dOut.data_ptr(), r.lbw.data_ptr(),
                                         r.saved.data_ptr(), r.scratch.data_ptr(), r.dX.data_ptr(), r.dY.data_ptr(), C.byref(r.gptrs), int(parts),
                                         torch.cuda.current_stream().cuda_stream)
        capi.check(st, f"avmoe_moe_backward_part({parts})")
        torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class Profiled:
    """the library's profiler around a site (no size threshold is lifted: the chain runs as the product path runs it)"""

    def __enter__(self):
        from avmoe_amd import _capi
        self.capi, self.L = _capi, _capi.lib()
        self.L.avmoe_prof_reset(); self.L.avmoe_prof_enable(1)
        return self

    def calls(self):
        """{kernel family: launches} since the last call"""
        torch.cuda.synchronize()
        ran = {f["name"]: int(f["calls"]) for f in self.capi.prof_report()}
        self.L.avmoe_prof_reset()
        return ran

    def __exit__(self, *exc):
        self.L.avmoe_prof_enable(0); self.L.avmoe_prof_reset()
        return False


class Recorder:
    def __init__(self, shape, family, dtype):
        self.key, self.fail = (shape, family, dtype), []

    def link(self, tag, kernel, fn):
        try:
            ratio = fn()
        except AssertionError as e:
            self.fail.append(f"{tag} [{kernel}]: {e}")
            return
        prev = CHECKED.setdefault(tag, {}).get(self.key)
        CHECKED[tag][self.key] = (kernel, max(ratio, prev[1] if prev else 0.0))
        print(f"MARGIN {tag} {' '.join(self.key)} {kernel} worst_err_over_bound {ratio:.4f}")

    def stepped_aside(self, tag, kernel, why):
        print(f"ASIDE  {tag} {' '.join(self.key)} {kernel} not launched: {why}")

    def finish(self):
        assert not self.fail, "\n".join(self.fail)


def _kernel_of(d, tag, fam, ran, rec, frames_seen):
    """the kernel family a link is counted under (asserted to have run); frames_seen collects the per-frame products gemm_frames served"""
    engine = sorted(n for n in ran if n.startswith("gemm") and not n.startswith("gemm_frames") and not n.startswith("gemm_stream"))
    if fam == "frames":
        link = "BmX" if tag == "BmX_pad" else tag
        served, form, why = H.frames_serves(d, link)
        if served:
            assert "gemm_frames" in ran, (tag, ran)
            frames_seen.add(link)
            TEXTS.add("gemm_frames " + form)
            return "gemm_frames " + form
        rec.stepped_aside(tag, "gemm_frames", why)
        stream = H.stream_serves(d, link)
        if stream:
            assert stream in ran, (tag, stream, ran)
            return stream
        assert engine, (tag, ran)
        return "engine"
    if fam == "gemm":
        assert engine, (tag, ran)
        return "engine"
    if fam in ran:
        return fam
    return fam + " (no profiler scope of its own)"         # k_finish_T / k_finish_dT / k_prep_dBm: launched unconditionally by the orchestration


def _run_links(s, B, links, ran, rec, count_frames=True):
    d = s.d
    frames_seen = set()
    for tag, (what, fam, fn) in links.items():
        kernel = _kernel_of(d, tag, fam, ran, rec, frames_seen)
        if tag in ("softmax", "softmax_x", "A1y_zeros"):
            text = H.softmax_text(d.N, d.Np)
            assert "k_softmax_rows" in ran, ran
            kernel = f"k_softmax_rows {text}"
            TEXTS.add("softmax fwd " + text)
        elif tag in ("softmax_bwd", "softmax_bwd_x"):
            text = H.softmax_bwd_text(d.Np)
            assert "k_softmax_rows_bwd" in ran, ran
            kernel = f"k_softmax_rows_bwd {text}"
            TEXTS.add("softmax bwd " + text)
        rec.link(tag, kernel, lambda fn=fn: fn(d, B))
    assert not count_frames or ran.get("gemm_frames", 0) == len(frames_seen), f"gemm_frames scopes {ran.get('gemm_frames', 0)}, products it serves here: {sorted(frames_seen)}; ran {sorted(ran.items())}"


def _once(s, prof, rec):
    """one forward + sectioned backward; rec: a Recorder on the first run, None on the repeat.  Returns the bytes of the checked buffers."""
    s.run.forward()
    ran = prof.calls()
    B = s.bufs()
    snap = s.raw(FWD_BUFS)
    snap["L1 forward"] = B["L1"][:, :s.d.Kcy, :s.d.N].clone()      # (its other entries: the workspace poison, then the first backward's dA1)
    if rec:
        H.check_family(s.d, B["L1"], rec.key[1])
        _run_links(s, B, H.FORWARD, ran, rec)
        # the NaN poison of the workspace is intact where no kernel of the forward writes: L1's row Kcy and its columns N .. Np
        d = s.d
        if not os.environ.get("AVMOE_TEST_ZERO_WS"):
            pad = torch.cat([B["L1"][:, d.Kcy].reshape(-1), B["L1"][:, :d.Kcy, d.N:].reshape(-1)])
            if not bool(torch.isnan(pad).all()):
                rec.fail.append(f"L1 padding: {int((~torch.isnan(pad)).sum())} of {pad.numel()} entries outside the product lost the workspace poison")
    s.begin_backward()
    s.part(1)
    s.part(32)
    ran = prof.calls()
    B = s.bufs()
    if rec:
        _run_links(s, B, {k: H.BACKWARD[k] for k in ("dTW", "dTT", "finish_dT")}, ran, rec)
    s.part(8)
    ran = prof.calls()
    if rec:
        _run_links(s, B, {k: v for k, v in H.BACKWARD.items() if k not in ("dTW", "dTT", "finish_dT")}, ran, rec)
    snap.update(s.raw(BWD_BUFS))
    for k in ("conv_adapter.weight", "conv_adapter.bias", "fc.weight", "fc.bias", *s.d.tok_keys):
        snap["grad " + k] = s.run.grads[k].clone()
    assert s.run.guards_intact(), "a kernel wrote past its workspace"
    return snap


@pytest.mark.parametrize("shape,family,dtype", CASES)
def test_hop1_chain_of_one_site(shape, family, dtype):
    S, N, M, E_m, E_s = SHAPES[shape]
    rec = Recorder(shape, family, dtype)
    with Profiled() as prof:
        s = Site(_cfg(N, M, E_m, E_s), S, family, bf16=dtype == "bf16")
        first = _once(s, prof, rec)
        second = _once(s, prof, None)
        for k, v in first.items():
            same = torch.equal(v.view(torch.uint8).reshape(-1), second[k].view(torch.uint8).reshape(-1))
            if not same:
                rec.fail.append(f"{k}: the second run of the site left other bytes")
    rec.finish()


V2_CASES = [("default", "bf16"), ("flat", "bf16"), ("peaked", "bf16"), ("default", "fp32")]


def _once_v2(s, prof, rec):
    """the AVS v2 site: the forward whole, the backward whole (the library does not split it: moe_backward.cpp:57-59)"""
    s.run.forward()
    ran = prof.calls()
    B = s.bufs()
    d = s.d
    snap = s.raw(FWD_BUFS + ("A1x",))
    snap["L1x"] = H._xview(d, B["L1"])[:, :, :d.N].clone()
    if rec:
        H.check_family(d, B["L1"], rec.key[1])
        _run_links(s, B, {**{k: H.FORWARD[k] for k in H.V2_FORWARD_Y}, **H.FORWARD_X}, ran, rec, count_frames=False)
    s.begin_backward()
    s.part(7)
    ran = prof.calls()
    B = s.bufs()
    if rec:
        _run_links(s, B, {**{k: H.BACKWARD[k] for k in H.V2_BACKWARD_Y}, **H.BACKWARD_X}, ran, rec, count_frames=False)
    snap.update(s.raw(tuple(k for k in BWD_BUFS if k != "L1") + ("dTx", "dL1xT")))
    snap["dA1x"] = H._xview(d, B["L1"])[:, :, :d.N].clone()
    for k in ("conv_adapter.weight", "conv_adapter.bias", "fc.weight", "fc.bias", *d.tok_keys):
        snap["grad " + k] = s.run.grads[k].clone()
    snap["dX"], snap["dY"] = s.run.dX.clone(), s.run.dY.clone()
    assert s.run.guards_intact(), "a kernel wrote past its workspace"
    return snap


@pytest.mark.parametrize("family,dtype", V2_CASES)
def test_hop1_chain_of_the_v2_site(family, dtype):
    """`g2c3_k20_v2` of tests/gen_pass_cases.py: K = 20 in 32-row slots (padding rows k >= K in A1y, A1x, Text, Tsum, T0T, dTW), latent self
    attention on X: A1x, the Text x slots through k_finish_T(src = 1), dTx, dA1x, dL1x and its transposed copy dL1xT (the only user of
    k_softmax_rows_bwd's out_t), dT0[x slots].  After the whole run L1 / TV / dL1 hold the x-side values: the y-side links that read them
    (L1, the y softmax per element, TV, k_finish_T on the y slots, dA1, the y softmax backward, dR^T, dWcK, k_dqrqb) are held at the other
    sites only; dX is out of scope (tests/test_stream_products_gpu.py: B3)."""
    from tests.gen_pass_cases import case_config
    cfg, S, seed, _fam, _inst = case_config("g2c3_k20_v2")
    rec = Recorder("v2_k20", family, dtype)
    with Profiled() as prof:
        s = Site(cfg, S, family, bf16=dtype == "bf16", seed=seed)
        assert s.d.Kp > s.d.K and s.d.Kcx > 0, (s.d.Kp, s.d.K, s.d.Kcx)
        first = _once_v2(s, prof, rec)
        second = _once_v2(s, prof, None)
        for k, v in first.items():
            if not torch.equal(v.view(torch.uint8).reshape(-1), second[k].view(torch.uint8).reshape(-1)):
                rec.fail.append(f"{k}: the second run of the site left other bytes")
    rec.finish()


def test_every_link_of_the_hop1_chain_was_checked():
    """Closes the module: every link was checked in at least two shapes, one of them ragged, and every kernel text / form was reached.  (Runs
    after the tests above: it fails when they did not run or a link was dropped.)"""
    missing = {}
    for tag in H.LINKS:
        got = {k[0] for k in CHECKED.get(tag, {})}
        only_v2 = tag in H.FORWARD_X or tag in H.BACKWARD_X          # (one site has latent self attention: its links count per family / dtype)
        if (len(CHECKED.get(tag, {})) < 2 if only_v2 else len(got) < 2) or not (got & RAGGED):
            missing[tag] = (H.LINKS[tag][0], sorted(got))
    for tag, sites in sorted(CHECKED.items()):
        for key, (kernel, ratio) in sorted(sites.items()):
            print(f"COVERED {tag} {' '.join(key)} {kernel} {ratio:.4f}")
    assert not missing, f"links not checked in two shapes (one ragged): {missing}"
    want = {"gemm_frames plain", "gemm_frames long", "gemm_frames long T", "gemm_frames plain T"}
    want |= {f"softmax {dr} {t}" for dr in ("fwd", "bwd") for t in ("reg4", "reg16", "plain")}
    assert want <= TEXTS, f"kernel texts / forms never reached: {sorted(want - TEXTS)}"
