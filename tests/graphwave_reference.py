"""What the GraphWave tests compare against: the fixtures of tests/golden/make_graphwave_golden.py (the reference's own runs) and
the dense float64 NumPy restatement of the contract (gcc_amd.graphwave.embed_numpy; the ``--device cpu`` path serves the same
function, and the CPU tier pins it to the fixtures)."""
import functools
import os

import numpy as np

from gcc_amd.graphwave import auto_taus, cheb_coefficients, embed_numpy, heat_numpy, live_nodes, time_points  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["n40d4", "n65d8", "n257d64", "n300d16", "hub300d8", "multi130d32", "n40d256", "task"]
EMU_FIXTURES = FIXTURES                                              # n <= 300 and d <= 64, plus n40d256
VARIANT_FACTOR = 16.0


def csr_from_edges(edges, n_rows):
    """symmetric CSR in node-id order with sorted rows from pairs u < v, a repeated pair a repeated entry
    -> (row_ptr int32, col_idx int32)"""
    both = np.concatenate([edges, edges[:, ::-1]]).astype(np.int64)
    both = both[np.lexsort((both[:, 1], both[:, 0]))]
    row_ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.add.at(row_ptr, both[:, 0] + 1, 1)
    return np.cumsum(row_ptr).astype(np.int32), both[:, 1].astype(np.int32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> dict(n_rows, d, edges, row_ptr, col_idx, chi, variant_distance[, heat_print, labels]); shared: do not write into its
    arrays"""
    z = np.load(os.path.join(GOLDEN, f"graphwave_{name}.npz"))
    fx = {k: z[k] for k in z.files}
    fx.update(n_rows=int(fx["n_rows"]), d=int(fx["d"]), variant_distance=float(fx["variant_distance"]))
    fx["row_ptr"], fx["col_idx"] = csr_from_edges(fx["edges"], fx["n_rows"])
    assert fx["variant_distance"] >= 0 and np.isfinite(fx["chi"]).all()
    return fx


@functools.lru_cache(maxsize=None)
def restatement(name):
    """``embed_numpy`` of the fixture, computed once; shared: do not write into its arrays"""
    fx = fixture(name)
    return embed_numpy(fx["row_ptr"], fx["col_idx"], fx["d"])
