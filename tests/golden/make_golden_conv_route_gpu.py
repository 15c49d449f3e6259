"""Records tests/golden/conv_route_gpu.json on an MI355X: `python tests/golden/make_golden_conv_route_gpu.py [out.json]`, with the
library and the icl_amd/ops.py of the commit whose calls are to be kept — the parent of the commit that introduced `ops.plan_conv3d`."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import pytest  # noqa: E402
import torch  # noqa: E402

import conv_route_checks as C  # noqa: E402

dev = torch.device("cuda", 0)
rows = C.record(pytest.MonkeyPatch, dev, C.CASES_GPU)
seen = set().union(*(C.forms_of(c, rows[C.case_id(c)]["trace"]) for c in C.CASES_GPU))
for c in C.CASES_GPU:
    print(C.case_id(c), sorted(C.forms_of(c, rows[C.case_id(c)]["trace"])))
print("unreached:", [f for f in C.FORMS_GPU if f not in seen])
with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_route_gpu.json"), "w") as f:
    f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n}\n")
print(len(rows), "rows")
