"""Driver for a kernel trace of top-p routing ("Top-p routing"):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o NAME -- python scripts/top_p_profile.py
    python scripts/top_p_profile.py --summarise OUT/.../NAME_kernel_trace.csv > per_shape.csv

Per (S, E) in (320, 4), (640, 4), (20480, 16), the shapes of scripts/sinkhorn_profile.py, on the same skewed softmax: --calls
avmoe_router_top_p calls (P = 0.9, k in [1, E], renorm, every output asked for: the apply launch and the count launch that reads its
bitmask), then --calls with the counts and no bitmask (the count launch selects on p itself), then --calls avmoe_router_sinkhorn calls
(k = 2, renorm, 4 rounds) -- kk_sk_apply of the same run is the yardstick of the apply launch.  The summary splits the per-dispatch rows
by that order (the first 5 calls of each group are warm-up and not counted)."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((320, 4), (640, 4), (20480, 16))
WARM = 5
TOP_P = 0.9


def run(calls):
    import torch
    from avmoe_amd import _capi as capi
    from tests import sinkhorn_ref as R
    L = capi.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for S, E in SHAPES:
        p = torch.from_numpy(R.family("skewed", S, E)).to(dev)
        w, v = torch.empty(S, E, device=dev), torch.empty(E, device=dev)
        choice, count = torch.empty(S, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
        khist = torch.empty(E + 1, dtype=torch.int32, device=dev)
        for bits in (choice.data_ptr(), None):
            for _ in range(calls):
                capi.check(L.avmoe_router_top_p(p.data_ptr(), S, E, TOP_P, 1, E, 1, None, w.data_ptr(), bits, count.data_ptr(), khist.data_ptr(), st),
                           "avmoe_router_top_p")
            torch.cuda.synchronize()
        print(f"top_p_profile: (S, E) = ({S}, {E}): frames per number of experts {khist.tolist()}")
        for _ in range(calls):
            capi.check(L.avmoe_router_sinkhorn(p.data_ptr(), S, E, 2, 1, 4, None, w.data_ptr(), choice.data_ptr(), count.data_ptr(), v.data_ptr(), st),
                       "avmoe_router_sinkhorn")
        torch.cuda.synchronize()
    print(f"top_p_profile: {calls} calls per (S, E) and form")


def summarise(path, calls):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
    out = csv.writer(sys.stdout)
    out.writerow(["kernel", "S", "E", "form", "workgroup", "grid", "calls", "mean_us", "min_us", "max_us"])
    for kern, forms in (("kk_top_p_apply", ("bitmask", "no bitmask")), ("kk_top_p_count", ("from the bitmask", "selects on p")),
                        ("kk_sk_scale", ("n = 4",)), ("kk_sk_apply", ("k = 2",))):
        mine = [r for r in rows if kern in r["Kernel_Name"]]
        assert len(mine) == calls * len(SHAPES) * len(forms), (kern, len(mine))
        for i, (S, E, form) in enumerate((S, E, form) for S, E in SHAPES for form in forms):
            grp = mine[i * calls + WARM:(i + 1) * calls]
            t = [us(r) for r in grp]
            out.writerow([kern, S, E, form, grp[0]["Workgroup_Size_X"], grp[0]["Grid_Size_X"], len(t), f"{sum(t) / len(t):.2f}", f"{min(t):.2f}", f"{max(t):.2f}"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=55)
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise is not None:
        summarise(a.summarise, a.calls)
    else:
        run(a.calls)
