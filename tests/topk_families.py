"""One adapter-site shape per bottleneck-space kernel family, and the family the library's plan puts a shape on -- read from the
workspace layout (avmoe_moe_buffer_info), so that a test can name the family it exercises without a GPU.  Shared by the top-k checks."""

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from oracle import avmoe_oracle as O
from tests.moe_gpu_util import make_desc

# family -> (AdapterConfig fields, frames, bf16)
FAMILIES = {
    # csrc/tile_stream.hip (kfs_*): the cfg-2 audio site in bf16; the plan gives it the register-resident shape, the streaming form is
    # chosen at launch (forced below its token threshold by the test hook; the profiler names its scopes "... (stream)")
    "tile_stream": (dict(Cx=768, Nx=1024, Cy=768, Ny=196, reduction=12, groups=2, K=32, variant="avs", lb_loss=True), 2, True),
    # csrc/tile_fast.hip (kf_*): register-resident, bottleneck 64 in two groups, 32 latent tokens, fp32
    "tile_fast": (dict(Cx=128, Nx=256, Cy=128, Ny=33, reduction=2, groups=2, K=32, variant="avs", lb_loss=True), 3, False),
    # csrc/tile_gen.inc (kg_*): the generalised kernels -- cfg-5 K = 87 (96 latent slots), four groups of 32, 4 + 4 experts
    "tile_gen": (dict(Cx=512, Nx=49, Cy=768, Ny=64, reduction=4, groups=4, K=87, variant="avs", E_m=4, E_s=4, lb_loss=True), 3, False),
    # csrc/tile_kernels.hip (kt_*): three groups of 8 (C = 480 > 384: not merged into one group), which no register-resident instance serves
    "tile_kernels": (dict(Cx=480, Nx=64, Cy=64, Ny=40, reduction=20, groups=3, K=8, variant="avs", lb_loss=True), 3, False),
}


def _ru(x, m):
    return (x + m - 1) // m * m


def plan_family(cfg, S, bf16, training=True):
    """'tile_fast' (the register-resident shape: tile_fast.hip, or tile_stream.hip when the streaming form is chosen at launch),
    'tile_gen' or 'tile_kernels', from the plan's layout (csrc/moe_plan.cpp):
      Wt  = g E dgp Cg elements            -> dgp, the padded per-group bottleneck
      mWd > 1 element                      -> the groups were merged into one (that site must be on the generalised kernels)
      a   = El NT Kp elements              -> Kp, the padded latent slot
    The generalised kernels pad dgp to 16 and the latent slots to 16 / 32 / 96; the any-shape kernels pad both to 8.  A shape where
    the two paddings coincide cannot be told apart: that raises."""
    assert cfg.self_attn == "none" and cfg.E_m > 0, "latent experts = the cross-modal ones"
    L = _capi.lib()
    d = make_desc(cfg, S, bf16, training)
    t = {n: b for (n, _r, _o, b) in cm.buffer_table(L, d)}
    esz = 2 if bf16 else 4
    E, C, NT = cfg.E, cfg.Cx, S * cfg.Nx
    dgp = t["Wt"] // (E * C * esz)
    merged = t["mWd"] > 4
    g = 1 if merged else cfg.groups
    Kp = t["a"] // (cfg.E_m * NT * esz)
    if g == 2 and dgp == 32 and cfg.K == 32 and Kp == 32 and 2 <= E <= 4:
        return "tile_fast"
    dg = cfg.d // g
    gen_kp = 16 if cfg.K <= 16 else (32 if cfg.K <= 32 else (96 if cfg.K <= 96 else _ru(cfg.K, 16)))
    gen = dgp == _ru(dg, 16) and Kp == gen_kp
    anyshape = dgp == _ru(dg, 8) and Kp == _ru(cfg.K, 8)
    if gen == anyshape:
        raise ValueError(f"the layout does not tell the families apart (dgp {dgp}, Kp {Kp}, merged {merged})")
    assert not (merged and anyshape), "a merged site runs on the generalised kernels"
    return "tile_gen" if gen else "tile_kernels"


def family_config(family):
    kw, S, bf16 = FAMILIES[family]
    return O.AdapterConfig(**kw), S, bf16
