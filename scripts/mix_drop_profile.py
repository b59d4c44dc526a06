"""Driver for a kernel trace of the mixture regularisers ("Stochastic depth and expert dropout on the mixture"):

    rocprofv3 --kernel-trace --stats -d OUT -o NAME -- python scripts/mix_drop_profile.py --drop-path 0.1 --expert-dropout 0.1

--steps pair steps (forward + backward of both AVE sites of the cfg-2 form through AdapterPair, two streams, bf16, 20 frames, training
mode), no warm-up apart: every step is in the trace, so the library's launches per site call are its calls / (2 * steps).  With both
rates 0 the sites run without the option (the `_aux` entry points); AVMOE_LIB may then point at an older library for the other side of a
comparison.  Prints one JSON line."""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def site(C, N, Cy, M, opt):
    from avmoe_amd.adapters import MoEAdapter
    return MoEAdapter(C, C, "bottleneck", None, 0, reduction_factor=12, opt=opt, use_bn=True, use_gate=True, num_tk=32, conv_dim_in=M,
                      conv_dim_out=N, linear_in=Cy, linear_out=C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--drop-path", type=float, default=0.0)
    ap.add_argument("--expert-dropout", type=float, default=0.0)
    a = ap.parse_args()
    from avmoe_amd.adapters import AdapterPair
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    opt = NS(num_conv_group=2, is_before_layernorm=1, is_post_layernorm=1, is_self_attention=0, num_multimodal_experts=2,
             num_singlemodal_experts=2, use_load_balacing_loss=0)
    sa, sv = site(768, 1024, 768, 196, opt).to(dev).train(), site(768, 196, 768, 1024, opt).to(dev).train()
    with torch.no_grad():
        for m in (sa, sv):
            for k, p in m.named_parameters():
                if k.endswith(("gate", "gate_av")):
                    p.fill_(0.3)
            m.drop_path, m.expert_dropout = a.drop_path, a.expert_dropout
    pair = AdapterPair(sa, sv)
    S = a.frames
    fa = (0.3 * torch.randn(S, 768, 1024, 1, device=dev)).bfloat16().requires_grad_(True)
    fv = (0.3 * torch.randn(S, 768, 196, 1, device=dev)).bfloat16().requires_grad_(True)
    ga, gv = torch.randn_like(fa), torch.randn_like(fv)
    for _ in range(a.steps):
        oa, _, ov, _ = pair(fa, fv)
        torch.autograd.backward([oa, ov], [ga, gv])
        fa.grad = fv.grad = None
        for m in (sa, sv):
            m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    print(json.dumps(dict(steps=a.steps, frames=S, drop_path=a.drop_path, expert_dropout=a.expert_dropout, lib=os.environ.get("AVMOE_LIB", "in-tree"),
                          mix_calls=[sa.mix_calls, sv.mix_calls])))


if __name__ == "__main__":
    main()
