"""Records tests/golden/conv_route.json: `python tests/golden/make_golden_conv_route.py path/to/libicl_emu.so`, with the emulation
library (tests/hipemu/build_emu.py) and the icl_amd/ops.py of the commit whose calls are to be kept — the parent of the commit that
introduced `ops.plan_conv3d`."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import pytest  # noqa: E402
import torch  # noqa: E402

from icl_amd import _lib  # noqa: E402

_lib._use_library_for_tests(os.path.abspath(sys.argv[1]), host_pointers=True)
import conv_route_checks as C  # noqa: E402

dev = torch.device("cpu")
rows = C.record(pytest.MonkeyPatch, dev, C.CASES_EMU)
seen = set().union(*(C.forms_of(c, rows[C.case_id(c)]["trace"]) for c in C.CASES_EMU))
assert not [f for f in C.FORMS_EMU if f not in seen], [f for f in C.FORMS_EMU if f not in seen]
rows["rng"] = C.rng_states(dev)
with open(os.path.join(HERE, "conv_route.json"), "w") as f:
    f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n}\n")
print(len(rows), "rows")
