"""The capacity rule of gcc_amd._cabi.bind_batch against the gfx950 library: on ``cuda`` tensors every engine refuses, by name and
before any launch, a batch one row short of its capacity; the accepted batch gives what the emulator gives.  The CPU tier
(recording stub, defaults, the host batcher) is tests/test_batch_binding_emu.py.

Tolerances: those of the engines' own device tests -- tests/test_encoder_gpu.py (rtol 1e-4, atol 2e-5), tests/wide_edges_check.py
(features: rtol 2e-4, atol 2e-5), tests/test_gat_gpu.py (rtol 1e-4, atol 1e-4), tests/wide_resident_reference.py (per-graph
relative distance below BAR_RULE; the emulator computes the bf16 rule)."""
import copy

import pytest
import torch

from tests import batch_binding_check as C
from tests.wide_resident_reference import BAR_RULE, graph_errors

pytestmark = pytest.mark.gpu

TOL = {"gin": dict(rtol=1e-4, atol=2e-5), "wide": dict(rtol=2e-4, atol=2e-5), "gat": dict(rtol=1e-4, atol=1e-4)}


@pytest.mark.parametrize("engine", list(C.ENGINES))
def test_engine_refuses_short_arrays_and_matches_the_emulator_on_the_accepted_batch(engine):
    from tests.hipemu.emu_driver import emu_lib

    enc = C.encoder(engine)
    want = C.call(engine, enc, C.batch(), lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr()).clone()
    dev = copy.deepcopy(enc).cuda()
    for field in C.ENGINES[engine][0]:
        C.refused(engine, dev, C.batch("cuda", short=field), field)
    got = C.call(engine, dev, C.batch("cuda"))
    torch.cuda.synchronize()
    got = got.cpu()
    print(f"{engine}: largest difference to the emulator {float((got - want).abs().max()):.2e} (largest entry {float(want.abs().max()):.2e})")
    if engine == "resident":
        err = graph_errors(got.numpy(), want.numpy())
        assert (err < BAR_RULE).all(), err
    else:
        torch.testing.assert_close(got, want, **TOL[engine])
