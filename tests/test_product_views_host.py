"""The matrix views of csrc/gemm.h (Mat) and the binding of a product to them (GemmArgs::product / add_segment / add_term), checked on the host:
tests/product_views_check.cpp builds one product per view operation -- T(), both sub-block forms, flat(), groups(), row blocks, planes, a
transposed C, a second segment, a D term -- and compares each with the descriptor written out by hand, field by field; then it provokes every
refusal (K, C shape, segment shape, element bytes against dtype / out_dtype, flat() of frames that do not abut).  CPU only: nothing is launched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = ["T() of B", "T() of A", "rows_at / cols_at (fp32)", "rows_at / cols_at (bf16)", "flat()", "groups()", "row_blocks()", "planes()", "frames_at()",
          "transposed C", "second segment + D term", "refuses: segment shape", "refuses: segment K", "refuses: D shape", "refuses: D element bytes",
          "refuses: K mismatch", "refuses: C shape (rows)", "refuses: C shape (columns)", "refuses: C not transposed", "refuses: A bytes vs dtype",
          "refuses: C bytes vs out", "refuses: flat() apart"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not cxx or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("no g++ / HIP headers on this box: the check program cannot be built here")
    exe = str(tmp_path_factory.mktemp("views") / "product_views_check")
    cmd = [cxx, "-std=c++17", "-O0", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), os.path.join(ROOT, "tests", "product_views_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def test_every_view_operation_and_refusal_holds(report):
    rc, out = report
    lines = out.strip().splitlines()
    assert rc == 0 and lines[-1] == "ok", out
    got = {ln[:28].strip(): ln[28:].strip() for ln in lines[:-1]}
    assert got == {name: "ok" for name in CHECKS}, out
