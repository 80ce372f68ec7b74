"""Writes tests/golden/ginw_forward_bits.npz: the outputs of gcc_ginw_forward (emulator build) on one batch of
tests/test_gin_wide_emu.py's generator, recorded BEFORE count_neighbours took an increment argument.  The batch has a
subgraph over 128 nodes, so both kernels (the fused one and the block-by-block one) are in it.
tests/test_wide_resident_emu.py compares today's outputs with these bit for bit.

    python -m tests.golden.make_ginw_forward_golden
"""
import hashlib
import os

import numpy as np

from oracle import gin_wide as ow
from tests.hipemu.emu_driver import emu_ginw_forward
from tests.test_gin_wide_emu import D, bits_layers, random_batch, random_layers

SIZES, DEG, L, SEED = [130, 37, 1, 64], 6, 2, 41
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ginw_forward_bits.npz")


def golden_inputs():
    rng = np.random.default_rng(SEED)
    layers = bits_layers(random_layers(rng, L))
    node_off, row_ptr, col_idx = random_batch(rng, SIZES, DEG)
    x = ow.to_bf16_bits(rng.standard_normal((int(node_off[-1]), D)).astype(np.float32))
    h = hashlib.sha256()
    for a in [node_off, row_ptr, col_idx, x] + [ly[k] for ly in layers for k in sorted(ly)]:
        h.update(np.ascontiguousarray(a).tobytes())
    return node_off, row_ptr, col_idx, x, layers, h.hexdigest()


if __name__ == "__main__":
    node_off, row_ptr, col_idx, x, layers, digest = golden_inputs()
    rows, pooled, status = emu_ginw_forward(node_off, row_ptr, col_idx, x, layers, scratch=True)
    assert status == 0
    np.savez_compressed(OUT, rows=rows, pooled=pooled, inputs_sha256=np.array(digest))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
