"""The sites of tests/test_gen_passes_fp64_gpu.py -- the generalised register-resident passes kg_* (csrc/tile_gen.inc) and the any-shape
passes kt_* / kk_mid (csrc/tile_kernels.hip, fwd_kernels.hip) -- with what can be said about them without a GPU: the layout the plan gives
each (read from avmoe_moe_buffer_info, as tests/topk_families.py does), the kernel family and (NG, NCG, KC) instance that follows from
it, and the rounds of resident experts each kernel runs (a transcription of pick_round / spread_rounds, tile_gen.inc:1005-1020, :1079-1081;
the product library has no switch that changes them).  tests/test_gen_pass_checker.py asserts this table on the CPU.

Where the plan puts a listed configuration on another instance or round size than the case is meant for, the configuration was changed
until the property is covered (what changed is said beside the case).  The frame lengths: per = the tokens of a block (moe_plan.cpp:169,
tile_gen.inc:984-988); blocks of fewer than 64 tokens get one resident expert (pick_round's `top`), so a case meant to have several
experts resident needs per >= 64: N in 49..64, 97..128, 193..256.
"""
from oracle import avmoe_oracle as O

# case -> (AdapterConfig fields, frames, seed, family, (NG, NCG, KC) or None for the any-shape form)
CASES = {
    # NCG = 1 (the odd chunk: ld_one / st_one), KC = 1 with 8 of 16 slots masked, five experts resident in ONE round (R = 5, NS = 1).
    # N: 70 -> 100 (70 gives blocks of 48 tokens: R = 1)
    "g2c1_k8_e5": (dict(Cx=96, Nx=100, reduction=3, groups=2, K=8, E_m=2, E_s=3), 3, 21, "tile_gen", (2, 1, 1)),
    # NCG = 3 (a chunk pair + an odd chunk; mmT_split's zero-padded half), KC = 2 unmasked; post_small / post_small_bwd / mid_bwd /
    # pre_small: R = 2 -> three rounds over grid.z; pre_lat_bwd: three latent slots in rounds of two -> an idle wave clamped to slot El - 1.
    # N: 130 -> 200 (130 gives blocks of 48 tokens)
    "g2c3_k32_e6": (dict(Cx=192, Nx=200, reduction=2, groups=2, K=32, E_m=3, E_s=3), 2, 21, "tile_gen", (2, 3, 2)),
    # KC = 2 with 12 of 32 slots masked; latent self attention: all four experts own a latent slot (the unimodal ones from X itself).
    # C, reduction: 96, 3 -> 192, 2 (96 / 3 is a bottleneck of 16 per group, NCG = 1).  Blocks of 48 tokens: R = 1, four rounds.
    "g2c3_k20_v2": (dict(Cx=192, Nx=77, reduction=2, groups=2, K=20, E_m=2, E_s=2, self_attn="v2", variant="avs"), 4, 21, "tile_gen", (2, 3, 2)),
    # NG = 4, KC = 6 (87 of 96 slots), the four-wave wide instance; mid / pre_small_bwd: R = 4 -> two rounds; post_small..: R = 2 -> four
    "g4c2_k87_e8": (dict(Cx=512, Nx=49, reduction=4, groups=4, K=87, E_m=4, E_s=4), 3, 21, "tile_gen", (4, 2, 6)),
    # NCG = 6; pre_small needs 120 192 B and pre_lat_bwd 115 600 B of dynamic LDS (> 64 KB: set_dyn_lds)
    "g2c6_k87": (dict(Cx=768, Nx=64, reduction=4, groups=2, K=87, E_m=4, E_s=4), 3, 21, "tile_gen", (2, 6, 6)),
    # 40 entries per group padded to 48.  E: 4 + 4 -> 4 + 3: seven experts in rounds of two (post_small, post_small_bwd, mid_bwd) leave
    # an idle wave in the last round, clamped to expert E - 1, rounds over grid.z
    "pad40_k87": (dict(Cx=320, Nx=100, reduction=4, groups=2, K=87, E_m=4, E_s=3), 3, 21, "tile_gen", (2, 3, 6)),
    # four groups of 3 merged into one group of 12 -> 16; K = 2 of 16 slots; three experts resident
    "merged_k2": (dict(Cx=96, Nx=100, reduction=8, groups=4, K=2, E_m=1, E_s=2, variant="avqa"), 4, 21, "tile_gen", (1, 1, 1)),
    # blocks of 48 tokens: R = 1, one expert per round, 24 entries per group padded to 32
    "short_36": (dict(Cx=768, Nx=36, reduction=8, groups=4, K=2, E_m=1, E_s=2, variant="avqa"), 4, 21, "tile_gen", (4, 2, 1)),
    # a frame shorter than one 16-token tile (the plan merges its two groups of 8)
    "tiny_3": (dict(Cx=64, Nx=3, reduction=4, groups=2, K=4, E_m=2, E_s=2), 5, 21, "tile_gen", (1, 1, 1)),
    # 384 blocks: the rounds run in the in-block loop e0 += R * gridDim.z.  C, reduction: 96, 3 -> 192, 2: at 16 entries per group every
    # kernel keeps all seven experts resident (one round, nothing to loop over); at 48, post_small / post_small_bwd / mid_bwd run four
    # rounds of two with an idle wave in the last.  Whole 16-token tiles.
    "many_blocks": (dict(Cx=192, Nx=64, reduction=2, groups=2, K=8, E_m=4, E_s=3), 384, 222, "tile_gen", (2, 3, 1)),
    # the any-shape form (tests/topk_families.py "tile_kernels": three groups of 8, C = 480 > 384 so not merged), whole and ragged tiles
    "kt_three_groups": (dict(Cx=480, Nx=64, Cy=64, Ny=40, reduction=20, groups=3, K=8, variant="avs", lb_loss=True), 3, 21, "tile_kernels", None),
    "kt_three_groups_50": (dict(Cx=480, Nx=50, Cy=64, Ny=40, reduction=20, groups=3, K=8, variant="avs", lb_loss=True), 3, 21, "tile_kernels", None),
}
BF16_CASES = ("g2c1_k8_e5", "g2c3_k32_e6", "g4c2_k87_e8", "g2c6_k87", "merged_k2", "many_blocks", "kt_three_groups", "kt_three_groups_50")
RAGGED = {c for c in CASES if c not in ("g2c6_k87", "many_blocks", "kt_three_groups")}      # (frames of 64 tokens: whole tiles)


def case_config(name):
    kw, S, seed, family, inst = CASES[name]
    kw = dict(kw)
    kw.setdefault("Cy", 64)
    kw.setdefault("Ny", 24)
    return O.AdapterConfig(**kw), S, seed, family, inst


def _ru(x, m):
    return -(-x // m) * m


class Layout:
    """What the plan decided for a site, read off the sizes of its workspace buffers ({name: bytes}): g (1 when the groups were merged), the
    padded entries per group dgp, the padded latent slots Kp, the element size of the Z-space tensors, and the family that follows."""

    def __init__(self, cfg, S, bf16, nbytes):
        E, NT = cfg.E, S * cfg.Nx
        self.esz = 2 if bf16 else 4
        self.merged = nbytes["mWd"] > 4                                     # (block-diagonal copies of down / up: moe_plan.cpp:95-105)
        self.g = 1 if self.merged else cfg.groups
        self.dg = cfg.d // self.g
        self.dgp = nbytes["wsum"] // 4 // (E * self.g)                      # wsum: DZ = E * g * dgp floats
        self.lat = list(range(E)) if cfg.self_attn == "v2" else list(range(cfg.E_m))      # the experts that own a latent slot, in slot order (moe_plan.cpp:82)
        self.El, self.K = len(self.lat), cfg.K
        self.Kp = nbytes["a"] // (self.El * NT * self.esz)
        self.zsz = nbytes["Z"] // (NT * E * self.g * self.dgp)
        self.KL = self.El * self.Kp
        self.KLT, self.KLp = self.KL + 2, _ru(self.KL + 2, 8)
        self.KP = E * self.dgp + 3 * E
        self.KPp = _ru(self.KP, 8)
        self.XW = _ru(self.KPp - E * self.dgp, 16)
        gen_kp = 16 if cfg.K <= 16 else (32 if cfg.K <= 32 else (96 if cfg.K <= 96 else _ru(cfg.K, 16)))
        gen = self.dgp == _ru(self.dg, 16) and self.Kp == gen_kp and self.zsz == self.esz          # moe_plan.cpp:126-130, :175
        anyshape = self.dgp == _ru(self.dg, 8) and self.Kp == _ru(cfg.K, 8) and self.zsz == 4
        tuned = self.g == 2 and self.dgp == 32 and cfg.K == 32 and 2 <= E <= 4
        assert not tuned and (gen or anyshape), f"neither family's layout (dgp {self.dgp}, Kp {self.Kp}, zsz {self.zsz})"
        if gen and anyshape:
            # an fp32 site whose two paddings coincide (entries per group a multiple of 16, 16 / 32 / 96 latent tokens): its own layout does
            # not tell the families apart.  The plan's choice reads no element size (moe_plan.cpp:126-130, tile_gen.inc:1063-1072), and the
            # bf16 layout of the same site does tell (Z in bf16 or in fp32): ask that one.
            assert not bf16
            gen = plan_layout(cfg, S, True).family == "tile_gen"
        self.family = "tile_gen" if gen else "tile_kernels"
        self.instance = (self.g, self.dgp // 16, self.Kp // 16) if gen else None
        # the tokens of a block (moe_plan.cpp:169, tile_gen.inc:984-988)
        N = cfg.Nx
        bps = max(1, min(-(-N // 64), max(-(-N // (256 if N >= 512 else 112)), -(-256 // S))))
        self.per, self.blocks = _ru(-(-N // bps), 16), bps * S


def plan_layout(cfg, S, bf16):
    """Layout of a site from the library's buffer table: no GPU needed"""
    from avmoe_amd import _capi
    from avmoe_amd import _capi_moe as cm
    from tests.moe_gpu_util import make_desc
    t = {n: b for (n, _r, _o, b) in cm.buffer_table(_capi.lib(), make_desc(cfg, S, bf16, True))}
    return Layout(cfg, S, bf16, t)


def _max_waves(ng, ncg, kc):                                                # gen_max_waves, tile_gen.inc:73
    return 4 if (ng * ncg >= 8 or kc == 6) else (16 if (ng * ncg <= 2 and kc <= 2) else 8)


def _pick_round(E, pe, pw, max_waves, per):                                 # pick_round, tile_gen.inc:1005-1020 (no development switch, excl = 0)
    top = 1 if per < 64 else min(E, max_waves)
    r = 1
    for c in (top, (top + 1) // 2, 2, 1):
        if c < 1 or c > E:
            continue
        ns = max(1, 4 // c)
        if c == 1 or (pe * c + pw * c * ns) * 4 <= 13 * 1024 * c * ns:
            r = c
            break
    ns = max(1, 4 // r)
    return r, ns, (pe * r + pw * r * ns) * 4


def rounds(lay, E):
    """{kernel: (R, NS, rounds, idle waves in the last round, dynamic LDS bytes, rounds in grid.z?)} of a generalised site, from the LDS
    each kernel's launcher asks pick_round for (tile_gen.inc:1098, :1122, :1148, :1177, :1221-1222, :1256, :1279)"""
    ng, ncg, kc = lay.instance
    GD, DD, Kp = lay.dgp, lay.g * lay.dgp, lay.Kp
    asks = {
        "pre_small": (E, Kp * (Kp + 4) + DD * (Kp + 4) + Kp + 2 * DD, DD, _max_waves(ng, ncg, kc)),
        "mid": (E, 2 * DD, DD, _max_waves(ng, ncg, 0)),
        "post_small": (E, DD * (GD + 4) + 4 * DD, 0, _max_waves(ng, ncg, 0)),
        "post_small_bwd": (E, DD * (GD + 4) + 4 * DD, DD + 1, _max_waves(ng, ncg, 0)),
        "mid_bwd": (E, DD * (GD + 4) + 5 * DD, DD, _max_waves(ng, ncg, 0)),
        "pre_small_bwd": (E, 7 * DD, DD + 1 + 64, _max_waves(ng, ncg, 0)),
        "pre_lat_bwd": (lay.El, Kp * (Kp + 4) + Kp * (DD + 4) + Kp, Kp + 1, _max_waves(ng, ncg, kc)),
    }
    out = {}
    for k, (n, pe, pw, mw) in asks.items():
        R, NS, lds = _pick_round(n, pe, pw, mw, lay.per)
        nr = -(-n // R)
        # kg_pre_small_bwd keeps its rounds in the block (its experts' sums meet in dsxs: tile_gen.inc:711); the others spread below 384 blocks
        out[k] = (R, NS, nr, nr * R - n, lds, lay.blocks < 384 and k != "pre_small_bwd")
    return out
