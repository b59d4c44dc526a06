"""Driver for a kernel trace of the expert capacity behind top-k routing ("Expert capacity"):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o NAME -- python scripts/capacity_profile.py
    python scripts/capacity_profile.py --summarise OUT/NAME_kernel_trace.csv > per_shape.csv

Per (S, E) in (320, 4), (640, 4), (20480, 16) and policy in (0 "order", 1 "priority"): --calls avmoe_router_capacity calls (k = 2,
c = ceil(k S / E): capacity factor 1, every output asked for) on a skewed softmax -- expert 0 is pushed up, so that it overflows and the
select runs all its passes while other experts stay within their budget --, then, as the yardstick, --calls avmoe_expert_choice calls at the
same c on the same matrix.  The summary splits the per-dispatch rows of kk_cap_mask / kk_cap_select / kk_cap_apply and of kk_ec_select /
kk_ec_apply by that order (the first 5 calls of each group are warm-up and not counted)."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((320, 4), (640, 4), (20480, 16))
POLICIES = (0, 1)
WARM = 5
K = 2


def skewed(S, E):
    import numpy as np
    z = 2.0 * np.random.default_rng(S + E).standard_normal((S, E))
    z[:, 0] += 1.5
    ez = np.exp(z - z.max(1, keepdims=True))
    return (ez / ez.sum(1, keepdims=True)).astype(np.float32)


def run(calls):
    import torch
    from avmoe_amd import _capi as capi
    from avmoe_amd.adapters import router_capacity
    L = capi.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for S, E in SHAPES:
        p = torch.from_numpy(skewed(S, E)).to(dev)
        c = router_capacity(1, K, S, E)
        w, cs, thr = torch.zeros(S, E, device=dev), torch.empty(S, E, device=dev), torch.empty(E, device=dev)
        kept = torch.empty(S, dtype=torch.int32, device=dev)
        demand, kc, last = (torch.empty(E, dtype=torch.int32, device=dev) for _ in range(3))
        for policy in POLICIES:
            for _ in range(calls):
                capi.check(L.avmoe_router_capacity(p.data_ptr(), S, E, K, None, c, policy, None, w.data_ptr(), cs.data_ptr(), kept.data_ptr(),
                                                   demand.data_ptr(), kc.data_ptr(), thr.data_ptr(), last.data_ptr(), st), "avmoe_router_capacity")
            torch.cuda.synchronize()
            print(f"capacity_profile: S {S} E {E} policy {policy} c {c} demand {demand.tolist()} kept {kc.tolist()}")
        for _ in range(calls):
            capi.check(L.avmoe_expert_choice(p.data_ptr(), S, E, c, 0, None, w.data_ptr(), kept.data_ptr(), thr.data_ptr(), last.data_ptr(), st),
                       "avmoe_expert_choice")
        torch.cuda.synchronize()
    print(f"capacity_profile: {calls} calls per (S, E, policy)")


def summarise(path, calls):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
    out = csv.writer(sys.stdout)
    out.writerow(["kernel", "S", "E", "policy", "workgroup", "grid", "calls", "mean_us", "min_us", "max_us"])

    def table(kern, groups):
        mine = [r for r in rows if kern in r["Kernel_Name"]]
        assert len(mine) == calls * len(groups), (kern, len(mine))
        for i, (S, E, pol) in enumerate(groups):
            grp = mine[i * calls + WARM:(i + 1) * calls]
            t = [us(r) for r in grp]
            out.writerow([kern, S, E, pol, grp[0]["Workgroup_Size_X"], grp[0]["Grid_Size_X"], len(t), f"{sum(t) / len(t):.2f}", f"{min(t):.2f}", f"{max(t):.2f}"])
    for kern in ("kk_cap_mask", "kk_cap_select", "kk_cap_apply"):
        table(kern, [(S, E, pol) for S, E in SHAPES for pol in POLICIES])
    for kern in ("kk_ec_select", "kk_ec_apply"):
        table(kern, [(S, E, "") for S, E in SHAPES])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=55)
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.calls)
    else:
        run(a.calls)
