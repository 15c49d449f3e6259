"""Records tests/golden/conv_plan.json: `python tests/golden/make_golden_conv_plan.py path/to/libicl_emu.so`, with the emulation
library (tests/hipemu/build_emu.py) of the commit whose answers are to be kept — the parent of the forward planner's commit."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from icl_amd import _lib  # noqa: E402
import test_conv_plan as T  # noqa: E402

_lib._use_library_for_tests(os.path.abspath(sys.argv[1]), host_pointers=True)
rows = T.table(_lib.lib(), os.environ.__setitem__, lambda k: os.environ.pop(k, None))
with open(os.path.join(HERE, "conv_plan.json"), "w") as f:
    f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n}\n")
print(len(rows), "rows")
