"""What the ProNE tests compare against: the fixtures of tests/golden/make_prone_golden.py (the reference's own runs), the
float64 NumPy / scipy.sparse restatement of the device's formulation (gcc_amd.prone.embed_numpy: Gram + ``eigh``, a QR normaliser,
the sign rule; the ``--device cpu`` path serves the same function, and the CPU tier pins it to the fixtures), and the same
pipeline with the reference's library calls (``embed_library``: sklearn's ``randomized_svd``, scipy's sparse products and
``scipy.linalg.svd``), which tools/prone_probe.py times."""
import functools
import os

import numpy as np

from gcc_amd.prone import bessel_iv, draw_omega, embed_numpy, flip_signs, node_terms, normalize_rows  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["n201d16", "n120d64", "n74d64", "n300d6", "n40d2", "hub", "task"]
EMU_FIXTURES = ["n201d16", "n300d6", "n40d2", "hub", "task"]             # n <= 300 and d <= 16
VARIANT_FACTOR = 16.0


def csr_from_edges(edges, n):
    """symmetric CSR in node-id order with sorted rows from pairs u < v -> (row_ptr int32, col_idx int32)"""
    both = np.concatenate([edges, edges[:, ::-1]]).astype(np.int64)
    order = np.lexsort((both[:, 1], both[:, 0]))
    both = both[order]
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(row_ptr, both[:, 0] + 1, 1)
    return np.cumsum(row_ptr).astype(np.int32), both[:, 1].astype(np.int32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> dict(n, d, seed, edges, row_ptr, col_idx, omega, emb_lu, emb_qr, emb_gesvd, variant_distance[, labels]); shared: do not
    write into its arrays"""
    z = np.load(os.path.join(GOLDEN, f"prone_{name}.npz"))
    fx = {k: z[k] for k in z.files}
    n, d, seed = int(fx["n"]), int(fx["d"]), int(fx["seed"])
    fx.update(n=n, d=d, seed=seed)
    fx["row_ptr"], fx["col_idx"] = csr_from_edges(fx["edges"], n)
    if "omega" not in fx:
        fx["omega"] = draw_omega(n, d, seed)
    lu = fx["emb_lu"]
    fx["variant_distance"] = max(float(np.abs(align(fx[a], fx[b]) - fx[b]).max())
                                 for a, b in (("emb_qr", "emb_lu"), ("emb_gesvd", "emb_lu"), ("emb_qr", "emb_gesvd")))
    assert fx["variant_distance"] > 0 and np.isfinite(lu).all()
    return fx


def align(emb, ref):
    """``emb`` with every column's sign turned to the one that is nearer to ``ref``'s (scipy.linalg.svd does not fix signs)"""
    flip = np.abs(emb + ref).sum(axis=0) < np.abs(emb - ref).sum(axis=0)
    return emb * np.where(flip, -1.0, 1.0)


def embed_library(row_ptr, col_idx, d, seed=0, step=5, mu=0.2, theta=0.5):
    """the reference's computation with its own library calls, on CSR arrays -> float64 [n, d]"""
    import scipy.sparse as sp
    from scipy import linalg
    from sklearn.utils.extmath import randomized_svd

    row_ptr, col_idx = np.asarray(row_ptr, dtype=np.int64), np.asarray(col_idx, dtype=np.int64)
    n = len(row_ptr) - 1
    deg, r, c = node_terms(row_ptr, col_idx)
    rows = np.repeat(np.arange(n), deg)
    F = sp.csc_matrix(sp.csr_matrix((r[rows] + c[col_idx], col_idx, row_ptr), shape=(n, n)))
    U, sigma, _ = randomized_svd(F, n_components=d, n_iter=5, random_state=np.random.RandomState(seed))
    a = normalize_rows(U * np.sqrt(sigma))
    if step == 1:
        return a
    A1 = sp.eye(n) + sp.csr_matrix((np.ones(len(col_idx)), col_idx, row_ptr), shape=(n, n))
    M = (1.0 - mu) * sp.eye(n) - sp.diags(1.0 / (deg + 1.0)) @ A1
    lx0, lx1 = a, 0.5 * (M @ (M @ a)) - a
    conv = bessel_iv(0, theta) * lx0 - 2 * bessel_iv(1, theta) * lx1
    for i in range(2, step):
        lx2 = (M @ (M @ lx1) - 2 * lx1) - lx0
        conv = conv + (2 if i % 2 == 0 else -2) * bessel_iv(i, theta) * lx2
        lx0, lx1 = lx1, lx2
    mm = A1 @ (a - conv)
    U, s, _ = linalg.svd(mm, full_matrices=False, check_finite=False)
    return normalize_rows(U[:, :d] * np.sqrt(s[:d]))
