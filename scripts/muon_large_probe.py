"""Times the large-matrix Newton-Schulz path of orthogonalised momentum alone (include/avmoe.h, avmoe_opt_muon_ns_large: block sums, normalise
and pack, three engine launches per iteration, unpack) against a torch restatement of the same five iterations on the same GPU.

    python scripts/muon_large_probe.py [--reps 30] [--runs 2] [--out FILE]

For each shape, for one matrix and for a class of 8: Gaussian values in one work buffer, five iterations, event-timed after five warm-up
launches, median / min / max of `reps` launches (the call re-normalises its input, so every call does the same work).  The yardstick is
torch: per matrix `X / (norm + 1e-7)`, then five times `A = X X^T; B = b A + c A A; X = a X + B X` with torch.mm in fp32, timed the same
way.  The two sides alternate, `runs` times each; every run is a line.  The torch loop is the yardstick, not the code under test: where
the library is slower the line says so and nothing here tunes anything."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(144, 160), (1024, 196), (768, 768), (1536, 768), (2304, 768)]
NS_A, NS_B, NS_C = 3.4445, -4.7750, 2.0315


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(1e3 * e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    L = capi.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"# lib {capi.LIB_PATH}  reps {a.reps}  runs {a.runs}  torch {torch.__version__}"]
    print(lines[0])
    for rows, cols in SHAPES:
        for copies in (1, 8):
            n = rows * cols
            stride = (n + 3) // 4 * 4
            g = torch.Generator().manual_seed(rows * 10007 + cols)
            buf = torch.randn(stride * copies, generator=g).to(dev)
            mats = (cm.OptMuonMat * copies)()
            for k, m in enumerate(mats):
                m.range, m.rows, m.cols = k, rows, cols
            lay = cm.OptMuonLargeLayout()
            assert L.avmoe_opt_muon_large_bytes(copies, mats, copies, C.byref(lay)) > 0
            img = torch.zeros(int(lay.table_bytes), dtype=torch.uint8)
            capi.check(L.avmoe_opt_muon_large_table_build(None, copies, mats, copies, None, 0, img.data_ptr(), int(lay.table_bytes)),
                       "avmoe_opt_muon_large_table_build")
            image = img.to(dev)
            ws = torch.zeros(int(lay.workspace_bytes), dtype=torch.uint8, device=dev)
            ptrs = torch.tensor([buf.data_ptr() + 4 * k * stride for k in range(copies)], dtype=torch.int64).to(dev)
            xs = [buf[k * stride:k * stride + n].view(rows, cols).clone() for k in range(copies)]

            def ours():
                capi.check(L.avmoe_opt_muon_ns_large(image.data_ptr(), img.data_ptr(), copies, ptrs.data_ptr(), 5, ws.data_ptr(), stream),
                           "avmoe_opt_muon_ns_large")

            def yardstick():
                for k in range(copies):
                    x = xs[k]
                    x = x / (torch.linalg.vector_norm(x) + 1e-7)
                    if rows > cols:
                        x = x.t()
                    for _ in range(5):
                        aa = torch.mm(x, x.t())
                        bb = torch.addmm(aa, aa, aa, beta=NS_B, alpha=NS_C)
                        x = torch.addmm(x, bb, x, beta=NS_A)
                    xs[k] = x.t().contiguous() if rows > cols else x

            d, ln = min(rows, cols), max(rows, cols)
            flop = 5 * (4.0 * d * d * ln + 2.0 * d ** 3) * copies
            for run in range(a.runs):
                for name, fn in (("library", ours), ("torch.mm", yardstick)):
                    med, lo, hi = timed(fn, a.reps)
                    line = (f"{rows:5d} x {cols:5d}  copies {copies}  run {run}  {name:8s}  median {med:9.1f} us  min {lo:9.1f}  max {hi:9.1f}  "
                            f"{flop / med / 1e3:9.1f} gflops")
                    print(line)
                    lines.append(line)
            sv = torch.linalg.svdvals(buf[:n].view(rows, cols).double().cpu())
            sy = torch.linalg.svdvals(xs[0].double().cpu())
            line = f"{rows:5d} x {cols:5d}  copies {copies}  singular values: library {float(sv.min()):.3f} .. {float(sv.max()):.3f}  torch {float(sy.min()):.3f} .. {float(sy.max()):.3f}"
            print(line)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
