"""Times the Newton-Schulz launch of orthogonalised momentum alone (include/avmoe.h, avmoe_opt_muon_ns): one workgroup per matrix.

    python scripts/muon_ns_probe.py [--copies 1] [--reps 30]

For each shape: `copies` matrices of Gaussian values in one work buffer, five iterations, event-timed after five warm-up launches,
median / min / max of `reps` launches (the launch re-normalises its input, so every launch does the same work).  AVMOE_LIB=<path> times
another build, e.g. one with -DMUON_GRAM_SECOND_PASS=1 (csrc/opt_muon.hip).  One line per shape; `gflops` counts
ns_steps * (4 d^2 L + 2 d^3) floating-point operations of the padded problem's useful part."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(4, 32), (32, 128), (87, 768), (768, 64), (64, 768), (96, 1536), (128, 128), (128, 1000), (128, 2048), (2048, 128)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=1)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    L = capi.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# lib {capi.LIB_PATH}  copies {a.copies}  reps {a.reps}")
    for rows, cols in SHAPES:
        n = rows * cols
        stride = (n + 3) // 4 * 4
        g = torch.Generator().manual_seed(rows * 10007 + cols)
        buf = torch.randn(stride * a.copies, generator=g).to(dev)
        mats = (cm.OptMuonMat * a.copies)()
        for k, m in enumerate(mats):
            m.range, m.rows, m.cols = k, rows, cols
        lay = cm.OptMuonLayout()
        assert L.avmoe_opt_muon_bytes(a.copies, 0, a.copies, C.byref(lay)) > 0
        img = torch.zeros(int(lay.table_bytes), dtype=torch.uint8)
        capi.check(L.avmoe_opt_muon_table_build(None, a.copies, mats, a.copies, img.data_ptr(), int(lay.table_bytes)), "avmoe_opt_muon_table_build")
        image = img.to(dev)
        ptrs = torch.tensor([buf.data_ptr() + 4 * k * stride for k in range(a.copies)], dtype=torch.int64).to(dev)

        def launch():
            capi.check(L.avmoe_opt_muon_ns(image.data_ptr(), a.copies, ptrs.data_ptr(), 5, stream), "avmoe_opt_muon_ns")

        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize()
            times.append(1e3 * e0.elapsed_time(e1))
        times.sort()
        d, ln = min(rows, cols), max(rows, cols)
        flop = 5 * (4.0 * d * d * ln + 2.0 * d ** 3) * a.copies
        med = times[len(times) // 2]
        sv = torch.linalg.svdvals(buf[:n].view(rows, cols).double().cpu())
        print(f"{rows:5d} x {cols:5d}  median {med:9.1f} us  min {times[0]:9.1f}  max {times[-1]:9.1f}  {flop / med / 1e3:8.1f} gflops  "
              f"singular values {float(sv.min()):.3f} .. {float(sv.max()):.3f}")


if __name__ == "__main__":
    main()
