"""dev: the record of tests/test_pass_forms_gpu.py -- per case, every profiler scope of one forward + backward with its call count and
algorithmic bytes (in name order) and a sha256 of out, probs, idx and of every gradient tensor.  Two builds that run the same forms on the same bits print the
same bytes:  AVMOE_LIB=<other build's libavmoe_hip.so> python tests/dev/pass_forms_record.py > record.txt   (needs an MI355X)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.test_pass_forms_gpu import CASES, digest, pass_scopes, run_case  # noqa: E402

for case in CASES:
    ran, guards, tensors = run_case(case)
    print(f"== {case}  hooks {'|'.join(CASES[case][1]) or 'none'}  guards {'intact' if guards else 'BROKEN'}")
    print("  passes: " + ", ".join(f"{n} x{c}" for n, c in sorted(pass_scopes(ran).items())))
    for n, (c, b) in sorted(ran.items()):
        print(f"  scope {n} x{c}  {b:.0f} bytes")
    for k, v in sorted(tensors.items()):
        print(f"  sha256 {k} {digest(v)}")
