"""The frame-attention ("v1") expert chain -- mha_frames_forward / mha_frames_backward (csrc/mha_frames.hip), about 25 launches per expert and
step -- and the x + xr glue it shares with the AVVP experts (k_xrstats, ZR = xr Wt^T, dxr = dZR Wt + rs xr, k_nxn_axpy), link by link against
fp64 of the link's own operands as stored in the workspace (tests/mha_ref.py: references, bounds, sites, input families;
tests/test_mha_checker.py shows on the CPU what such a check catches).  One site per case (NaN-poisoned workspaces, guard bands), one Recorder
per site: a run reports every failing link.

The forward runs whole; the scores (mSc) are read behind it, before the backward overwrites them with dPd.  The backward runs in sections 1, 2, 4
(avmoe_moe_backward_part) and is read after 2.  Every site runs twice: the checked buffers hold the same bytes; the guard bands are intact.

Sites (mha_ref.SITES), variant avs, self_attn v1, 2 groups unless said otherwise:
  S5_C64     S = 5 < Sp = 8, the fixtures' shape; bf16 and fp32
  S8_C32     S == Sp; dh = 8; N = 25 odd; 3 C = 96 leaves a partial 64-column block in km_colsum_part; NT = 200: three row chunks
  S13_C96    Sp = 16, two 8-groups; dh = 24: a K tail in q k^T; bf16 and fp32; the flat and the peaked family
  S70_C128   S above a 64-row tile and a 64-wide softmax row (kk_softmax_rows_reg<T, 4> all the same: a lane holds 16 entries, mha_ref SOFTMAX);
             the flat and the peaked family
  S13_C320   dh = 80, a production width
  S13_two_slots   E_m = E_s = 2: the forward of both slots (slot 0's softmax from fp64 scores with the product's bound, its scores being
             overwritten by slot 1's); the backward of the last slot and that expert's gradients.  Slot 0's backward scratch is NOT held.
  S5_eval    eval mode: no sa_keep, mPd untouched (the workspace poison), forward only
  avvp       variant avvp, S = 6, N = 40, C = 96, E 2 + 2: the glue links with the whole-Wt dxr, k_nxn_axpy(replaces = 0), one shared xr slot

Every training site has a drawn keep multiplier in {0, 1 / 0.8} with one all-zero row per expert (mha_ref.draw_keep).  The families' conditions
are asserted from the stored scores (mha_ref.check_family); measured on the GPU's stored mSc (profiles/r32_mha_chain_margins.txt):
  S13_C96 flat: max span 0.015; peaked: 0.978 of the rows span > 8, row maxima 0.333 column 0 / 0.333 column S - 1 / 0.667 last 8-group
  S70_C128 flat: max span 0.021; peaked: 1.000 of the rows span > 8, row maxima 0.333 column 0 / 0.320 column S - 1 / 0.590 last 8-group

The profiler report must show mha_frames_forward, k_xrstats (forward) and k_nxn_axpy, mha_frames_backward (section 2) once per slot.  A
profiler record ends with the first scope that closes (csrc/prof.cpp:39, :58), so the record named mha_frames_* covers the stage up to its
first scoped launch (k_cast; in the backward the dWout product) and every later product of the stage shows under the name of the kernel that
served it.  WHICH kernel serves each product is asserted per site, exactly, tile included: mha_ref.stage_instances transcribes launch_gemm's
order -- the B-stationary streaming kernel first (gemm_stream.hip:591-599, :721-727), never gemm_frames, then the tile the block count picks
(gemm.hip:1176-1180) -- and every v1 site runs beside a TWIN, the same site without self attention (same shapes, same plan otherwise): the
difference of the two reports' gemm* records must be exactly the predicted instances.  What follows from the transcription:
  * the batched per-(token, head) products (q k^T, Pd v, dO v^T, Pd^T dO, dS k, dS^T q) are engine instances of the 32 tile at every site here
    (S = 70 too: 2 x 2 x 24 blocks of the 64 tile are fewer than 160);
  * the flat NT-row products with a K-major A (X Win^T, O Wout^T, ZR, dxr, dxr Wout) leave the engine for gemm_stream_* at the bf16 sites
    with NT >= 256: S70_C128 (k160_n384; k64_n192 for the glue) and S13_two_slots (k64_n192);
  * dX += dQKV Win accumulates and has K = 3 C: the streaming kernel steps aside (its k384_n128 form does not accumulate) and the engine
    runs it.  The streaming kernel used to leave a profiler record named gemm_stream_k384_n128 for this product WITHOUT a launch (the scope
    opened before the form stepped aside); found here, fixed in gemm_stream.hip (STREAM_CASE);
  * fp32 sites: the stage runs the exact fp32 instances (split3 = 0), the glue three planes.
The AVVP site's glue products are printed as ENGINE lines only (its twin would differ by the whole N x N block).
"""
import os

import pytest
import torch

from oracle import avmoe_oracle as O
from tests import hop1_ref as H
from tests import mha_ref as M
from tests.test_hop1_chain_fp64_gpu import Profiled
from tests.test_hop1_chain_fp64_gpu import Site as HopSite

pytestmark = pytest.mark.gpu

CHECKED = {}      # link -> {(site, family, dtype): worst err / bound}
FWD_BUFS = ("mWin", "mWout", "mQKV", "mP", "mO", "xr", "sxr")
BWD_BUFS = ("dxr", "mSc", "mdO", "mdS", "mdQKV")
ZEROED = bool(os.environ.get("AVMOE_TEST_ZERO_WS"))


class Site(HopSite):
    """one site of mha_ref.SITES on cuda:0 (tests/moe_gpu_util.py::MoeRun with mha_keep) and every buffer of the chain as a typed device view"""

    def __init__(self, site, family, dtype):
        from tests.moe_gpu_util import MoeRun
        cfg, S, training, P, Bf, X, Y, G, keep = M.draw_site(site, family)
        self.cfg, self.S, self.G, self.training = cfg, S, G, training
        self.run = MoeRun(cfg, P, Bf, X, Y, bf16=dtype == "bf16", training=training, mha_keep=keep)
        self.d = M.Dims(cfg, S, dtype == "bf16", {k: v[2] for k, v in self.run.table.items()})
        self.keep = None if keep is None else {k: v.to(self.run.dev) for k, v in keep.items()}

    def bufs(self):
        B = super().bufs()
        B["keep"], B["dX"] = self.keep, getattr(self.run, "dX", None)
        return B


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class Recorder:
    def __init__(self, key):
        self.key, self.fail = key, []

    def link(self, tag, kernel, fn):
        try:
            ratio = fn()
        except AssertionError as e:
            self.fail.append(f"{tag} [{kernel}]: {e}")
            return
        CHECKED.setdefault(tag.split("[")[0], {})[self.key + (tag,)] = ratio
        print(f"MARGIN {tag} {' '.join(self.key)} {kernel} worst_err_over_bound {ratio:.4f}")

    def expect(self, ok, what):
        if not ok:
            self.fail.append(what)

    def finish(self):
        assert not self.fail, "\n".join(self.fail)


def _engines(ran):
    return " ".join(f"{k}x{v}" for k, v in sorted(ran.items()) if k.startswith("gemm"))


class Twin(HopSite):
    """the same site without self attention: what its profiler report lacks against the v1 site's is the stage and its glue"""

    def __init__(self, site, dtype):
        import dataclasses
        from tests.moe_gpu_util import MoeRun
        cfg, S, training = M.site_config(site)
        cfg = dataclasses.replace(cfg, self_attn="none")
        P, Bf = O.init_params(cfg, seed=M.SEED)
        g = torch.Generator().manual_seed(M.SEED + 100)
        X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
        Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
        self.G = torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
        self.cfg, self.S, self.training = cfg, S, training
        self.run = MoeRun(cfg, P, Bf, X, Y, bf16=dtype == "bf16", training=training)
        self.d = H.Dims(cfg, S, dtype == "bf16", {k: v[2] for k, v in self.run.table.items()})


def _gemms(ran):
    return {k: v for k, v in ran.items() if k.startswith("gemm")}


def twin_records(site, dtype, prof):
    """(gemm* records of the twin's forward, of its section 2)"""
    t = Twin(site, dtype)
    t.run.forward()
    fwd = _gemms(prof.calls())
    if not t.training:
        return fwd, {}
    t.begin_backward()
    t.part(1)
    prof.calls()
    t.part(2)
    sec2 = _gemms(prof.calls())
    t.part(4)
    prof.calls()
    return fwd, sec2


def _expect_instances(rec, ran, twin, want, where):
    """the v1 site's gemm* records minus its twin's: exactly the predicted instances of the stage and its glue"""
    got = {k: v - twin.get(k, 0) for k, v in _gemms(ran).items() if v != twin.get(k, 0)}
    got.update({k: -v for k, v in twin.items() if k not in ran})
    print(f"STAGE {where} {' '.join(rec.key)} " + " ".join(f"{k}x{v}" for k, v in sorted(got.items())))
    rec.expect(got == want, f"{where}: the stage and its glue ran as {sorted(got.items())}, launch_gemm's order says {sorted(want.items())}")


def _once(s, prof, rec, twin=None):
    """one forward + sectioned backward; rec: a Recorder on the first run, None on the repeat.  Returns the bytes of the checked buffers."""
    d = s.d
    nslots = len(d.slots) if d.v1 else 1
    last = d.slots[-1][0]
    s.run.forward()
    ran = prof.calls()
    B = s.bufs()
    if d.v1:
        B["scores"] = B["mSc"].clone()
    snap = s.raw(tuple(k for k in FWD_BUFS if d.v1 or not k.startswith("m")) + ("ZR",))
    if d.v1:
        snap["scores"] = B["scores"]
        snap["mPd"] = s.raw(("mPd",))["mPd"]
    if rec:
        print(f"ENGINE forward {' '.join(rec.key)} {_engines(ran)}")
        rec.expect(ran.get("k_xrstats", 0) == nslots, f"k_xrstats ran {ran.get('k_xrstats', 0)} times for {nslots} xr slots: {sorted(ran.items())}")
        if d.v1:
            rec.expect(ran.get("mha_frames_forward", 0) == nslots, f"mha_frames_forward ran {ran.get('mha_frames_forward', 0)} times for {nslots} slots: {sorted(ran.items())}")
            _expect_instances(rec, ran, twin[0], M.stage_instances(d)[0], "forward")
            # mSc ends with its last matrix: whatever the table rounds its size up by is untouched
            region, off, nbytes = s.run.table["mSc"]
            tail = s.run.scratch[off + 4 * d.N * d.H * d.S * d.Sp:off + nbytes]
            rec.expect(bool((tail == (0 if ZEROED else 0xFF)).all()), f"mSc: {int((tail != (0 if ZEROED else 0xFF)).sum())} of {tail.numel()} bytes behind the last matrix were written")
            got = M.check_family(d, B["scores"], rec.key[1])
            print(f"FAMILY {' '.join(rec.key)} " + ", ".join(f"{a} {b:.3f}" for a, b in got.items()))
            for j, _e, _pre in d.slots:
                for tag, (_what, kernel, fn) in M.FORWARD.items():
                    kw = {"stored_scores": j == last} if tag == "softmax" else ({"zeroed": ZEROED} if tag == "keep" else {})
                    rec.link(f"{tag}[{j}]", kernel + (" reg4" if tag == "softmax" else ""), lambda fn=fn, j=j, kw=kw: fn(d, B, j, **kw))
            rec.link("scores", "gemm", lambda: M.link_scores(d, B, last, ZEROED))
            rec.link("zr_others", "none", lambda: M.link_zr_others(d, B, ZEROED))
        else:
            for tag in ("sxr", "zr"):
                rec.link(tag, M.FORWARD[tag][1], lambda tag=tag: M.FORWARD[tag][2](d, B, 0))
    if not s.training:
        assert s.run.guards_intact(), "a kernel wrote past its workspace"
        return snap
    s.begin_backward()
    s.part(1)
    prof.calls()
    s.part(2)
    ran = prof.calls()
    B2 = s.bufs()
    B2["scores"] = B.get("scores")
    if rec:
        print(f"ENGINE section2 {' '.join(rec.key)} {_engines(ran)}")
        rec.expect(ran.get("k_nxn_axpy", 0) == nslots, f"k_nxn_axpy ran {ran.get('k_nxn_axpy', 0)} times for {nslots} xr slots: {sorted(ran.items())}")
        if d.v1:
            rec.expect(ran.get("mha_frames_backward", 0) == nslots, f"mha_frames_backward ran {ran.get('mha_frames_backward', 0)} times for {nslots} slots: {sorted(ran.items())}")
            _expect_instances(rec, ran, twin[1], M.stage_instances(d)[1], "section 2")
            for tag, (_what, kernel, fn) in M.BACKWARD.items():
                if tag == "dx" and nslots > 1:
                    continue                                       # (two slots: dX also holds slot 0's three terms, whose operands are gone)
                kw = {"zeroed": ZEROED} if tag == "dpd" else {}
                rec.link(tag, kernel + (" reg4" if tag == "ds" else ""), lambda fn=fn, kw=kw: fn(d, B2, last, **kw))
            # the caller's gradients of the self attention: the NaN prefill is gone in every element of EVERY v1 expert
            for _j, _e, pre in d.slots:
                for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
                    g = s.run.grads[f"{pre}.self_attention.{k}"]
                    rec.expect(bool(torch.isfinite(g).all()), f"{pre}.self_attention.{k}: {int((~torch.isfinite(g)).sum())} elements of the gradient not written")
        else:
            rec.link("dxr", M.BACKWARD["dxr"][1], lambda: M.link_dxr(d, B2, 0))
    snap.update(s.raw(tuple(k for k in BWD_BUFS if d.v1 or not k.startswith("m"))))
    if d.v1:
        for _j, _e, pre in d.slots:
            for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
                snap[f"grad {pre}.{k}"] = s.run.grads[f"{pre}.self_attention.{k}"].clone()
        snap["dX behind section 2"] = s.run.dX.clone()
    s.part(4)
    assert s.run.guards_intact(), "a kernel wrote past its workspace"
    return snap


@pytest.mark.parametrize("site,family,dtype", M.CASES)
def test_mha_chain_of_one_site(site, family, dtype):
    rec = Recorder((site, family, dtype))
    with Profiled() as prof:
        twin = twin_records(site, dtype, prof) if M.SITES[site][7] == "v1" else None
        s = Site(site, family, dtype)
        first = _once(s, prof, rec, twin)
        second = _once(s, prof, None)
        for k, v in first.items():
            if not torch.equal(v.contiguous().view(torch.uint8).reshape(-1), second[k].contiguous().view(torch.uint8).reshape(-1)):
                rec.fail.append(f"{k}: the second run of the site left other bytes")
    rec.finish()


def test_every_link_of_the_mha_chain_was_checked():
    """Closes the module (runs after the tests above: it fails when they did not run or a link was dropped): every link at every v1 training
    site, the forward links at both slots of the two-slot site and at the eval site, the glue links at the AVVP site."""
    v1_train = {c for c in M.CASES if M.SITES[c[0]][7] == "v1" and M.SITES[c[0]][8]}
    missing = {}
    for tag in list(M.FORWARD) + ["scores", "zr_others"]:
        want = {c for c in M.CASES if M.SITES[c[0]][7] == "v1"} | ({("avvp", "default", "bf16")} if tag in M.GLUE else set())
        got = {k[:3] for k in CHECKED.get(tag, {})}
        if want - got:
            missing[tag] = sorted(want - got)
    for tag in M.BACKWARD:
        want = {c for c in v1_train if not (tag == "dx" and c[0] == "S13_two_slots")} | ({("avvp", "default", "bf16")} if tag in M.GLUE else set())
        got = {k[:3] for k in CHECKED.get(tag, {})}
        if want - got:
            missing[tag] = sorted(want - got)
    two = {k[3] for tag in M.FORWARD for k in CHECKED.get(tag, {}) if k[0] == "S13_two_slots"}
    assert not missing, f"links not checked: {missing}"
    assert {f"{t}[{j}]" for t in M.FORWARD for j in (0, 1)} <= two, sorted(two)
