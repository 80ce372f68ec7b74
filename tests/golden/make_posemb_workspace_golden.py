"""Records gcc_posemb_multi_workspace_bytes (emulator library, default grid caps, hidden 32) for the shapes of
tests/test_posemb_emu.py::test_workspace_sizes_are_the_recorded_ones into tests/golden/posemb_workspace_bytes.json.
Callers cache these sizes, so a change of the workspace layout must keep them: run this at the commit BEFORE such a
change, from the repository root (python -m tests.golden.make_posemb_workspace_golden)."""
import json
import os

from tests.hipemu.emu_driver import emu_lib

SHAPES = [(1, 6, 6 * 257), (1, 8, 8 * 1025), (3, 4, 4 * 257), (16, 256, 256 * 257)]

os.environ.pop("GCC_POSEMB_GRID_CAPS", None)
os.environ.pop("GCC_POSEMB_GATED_CAPS", None)
lib = emu_lib()
rows = [dict(views=v, batch_size=b, node_cap=c, hidden=32, bytes=int(lib.gcc_posemb_multi_workspace_bytes(v, b, c, 32)))
        for v, b, c in SHAPES]
json.dump(rows, open(os.path.join(os.path.dirname(__file__), "posemb_workspace_bytes.json"), "w"), indent=1)
print(rows)
