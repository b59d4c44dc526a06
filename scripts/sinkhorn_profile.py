"""Driver for a kernel trace of Sinkhorn-balanced routing ("Sinkhorn-balanced top-k routing"):

    rocprofv3 --kernel-trace --stats -d OUT -o NAME -- python scripts/sinkhorn_profile.py
    python scripts/sinkhorn_profile.py --summarise OUT/.../NAME_kernel_trace.csv > per_shape.csv

Per (S, E) in (320, 4), (640, 4), (20480, 16) and n in (4, 8): --calls avmoe_router_sinkhorn calls (k = 2, renorm, every output asked
for) on a skewed softmax, in that order; then --router-calls avmoe_router_forward calls -- the site's router forward as a whole: the
layer-1 product, the tail kernel, the load-balancing loss -- at S = 20480, E = 16 on a site with 128 channels and 8 tokens (the
workspace of a 768-channel site at that S takes tens of GB; its layer-1 product is six times this one's).  The summary splits the
per-dispatch rows of kk_sk_scale / kk_sk_apply by that order (the first 5 calls of each group are warm-up and not counted) and sums the
kernels of each router forward."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((320, 4), (640, 4), (20480, 16))
ITERS = (4, 8)
WARM = 5
ROUTER_S, ROUTER_E = 20480, 16


def run(calls, router_calls):
    import ctypes as C
    import torch
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    from oracle import avmoe_oracle as O
    from tests import sinkhorn_ref as R
    from tests.moe_gpu_util import make_desc
    L = capi.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for S, E in SHAPES:
        p = torch.from_numpy(R.family("skewed", S, E)).to(dev)
        w, v = torch.empty(S, E, device=dev), torch.empty(E, device=dev)
        choice, count = torch.empty(S, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
        for n in ITERS:
            for _ in range(calls):
                capi.check(L.avmoe_router_sinkhorn(p.data_ptr(), S, E, 2, 1, n, None, w.data_ptr(), choice.data_ptr(), count.data_ptr(),
                                                   v.data_ptr(), st), "avmoe_router_sinkhorn")
            torch.cuda.synchronize()
    cfg = O.AdapterConfig(Cx=128, Nx=8, Cy=128, Ny=8, reduction=4, groups=2, K=8, variant="avs", E_m=ROUTER_E // 2, E_s=ROUTER_E // 2, lb_loss=True)
    P, _B = O.init_params(cfg, seed=3)
    params = {k: t.to(dev).float().contiguous() for k, t in P.items()}
    ptrs = cm.make_ptrs(params, cfg.E_m, cfg.E_s)
    d = make_desc(cfg, ROUTER_S, False, True)
    saved = torch.empty(L.avmoe_moe_saved_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
    scratch = torch.empty(L.avmoe_moe_scratch_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
    rin = 0.3 * torch.randn(ROUTER_S, 2 * cfg.Cx, device=dev)
    probs, idx = torch.empty(ROUTER_S, ROUTER_E, device=dev), torch.empty(ROUTER_S, dtype=torch.int64, device=dev)
    lb = torch.empty((), device=dev)
    for _ in range(router_calls):
        capi.check(L.avmoe_router_forward(C.byref(d), rin.data_ptr(), C.byref(ptrs), None, probs.data_ptr(), idx.data_ptr(), lb.data_ptr(),
                                          saved.data_ptr(), scratch.data_ptr(), st), "avmoe_router_forward")
    torch.cuda.synchronize()
    print(f"sinkhorn_profile: {calls} calls per (S, E, n), {router_calls} router forwards")


def summarise(path, calls):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
    out = csv.writer(sys.stdout)
    out.writerow(["kernel", "S", "E", "iters", "workgroup", "grid", "calls", "mean_us", "min_us", "max_us"])
    for kern in ("kk_sk_scale", "kk_sk_apply"):
        mine = [r for r in rows if kern in r["Kernel_Name"]]
        assert len(mine) == calls * len(SHAPES) * len(ITERS), (kern, len(mine))
        for i, (S, E, n) in enumerate((S, E, n) for S, E in SHAPES for n in ITERS):
            grp = mine[i * calls + WARM:(i + 1) * calls]
            t = [us(r) for r in grp]
            out.writerow([kern, S, E, n, grp[0]["Workgroup_Size_X"], grp[0]["Grid_Size_X"], len(t), f"{sum(t) / len(t):.2f}", f"{min(t):.2f}", f"{max(t):.2f}"])
    # the router forwards: everything dispatched behind the last Sinkhorn kernel, split at each kk_router_tail's successor (kk_lb_loss ends a call)
    last = max(i for i, r in enumerate(rows) if "kk_sk_" in r["Kernel_Name"])
    tail = [r for r in rows[last + 1:] if "avmoe" in r["Kernel_Name"]]
    ends = [i for i, r in enumerate(tail) if "kk_lb_loss" in r["Kernel_Name"]]
    per_call, start = [], 0
    for e in ends:
        per_call.append(sum(us(r) for r in tail[start:e + 1]))
        start = e + 1
    t = per_call[WARM:]
    out.writerow(["k_router (all its kernels)", ROUTER_S, ROUTER_E, "", "", "", len(t), f"{sum(t) / len(t):.2f}", f"{min(t):.2f}", f"{max(t):.2f}"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=55)
    ap.add_argument("--router-calls", type=int, default=25)
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.calls)
    else:
        run(a.calls, a.router_calls)
