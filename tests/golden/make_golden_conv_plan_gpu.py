"""Records tests/golden/conv_plan_gpu.json on an MI355X: `ICL_HIP_LIB=path/to/libicl_hip.so python tests/golden/make_golden_conv_plan_gpu.py
[out.json]`, with the library of the commit whose launches are to be kept — the parent of the forward planner's commit."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import test_gpu_conv_plan as T  # noqa: E402

for k in [k for k in os.environ if k.startswith(("ICL_CONV_", "ICL_WGRAD_"))]:
    del os.environ[k]
dev = torch.device("cuda", 0)
numel = max(2 * max(cin, cout) * e ** 3 for cin, cout, e in T.LAYERS)
pool = {"x": T._fill(numel, 1, dev), "gy": T._fill(numel, 2, dev)}
rows = {f"{cin}|{cout}|{e}": T.launch_record(dev, cin, cout, e, pool) for cin, cout, e in T.LAYERS}
with open(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN, "w") as f:
    f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n}\n")
print(len(rows), "rows")
