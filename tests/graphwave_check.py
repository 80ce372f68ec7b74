"""The GraphWave kernels (gcc_amd/csrc/graphwave.hip) against the reference's own runs (tests/golden/graphwave_*.npz) and the NumPy
restatement, shared by the emulator tier (tests/test_graphwave_emu.py) and the GPU tier (tests/test_graphwave_gpu.py): the same
cases and checks; only the library, the pointer function and the device differ.

Tolerances.  Whole table: max|chi - reference| <= 16 x the fixture's ``variant_distance`` (the larger of the reference's distance
from itself under relabelling and from the same formulas in long double; 16 is the factor of the ProNE checks), and the same
against the restatement.  Heat stage: the set of zeroed entries is the reference's exactly (the generating script asserts that no
entry lies within a relative 1e-6 of the threshold), and a kept entry is within 31 (deg_max + 2) 2^-52 sum_k |c_k| of the
reference's: 31 terms in another order, each a product over at most deg_max neighbours."""
import ctypes

import numpy as np
import pytest
import torch

from gcc_amd import _cabi
from gcc_amd.graphwave import GraphWaveEngine
from tests import graphwave_reference as R

EPS = 2.0 ** -52


class Gw:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors)"""

    def __init__(self, lib, ptr, device):
        self.lib, self.ptr, self.device = lib, ptr, torch.device(device)
        self.engine = GraphWaveEngine(lib, ptr, device)

    def embed(self, row_ptr, col_idx, d, **kw):
        return {k: v.cpu().numpy() for k, v in self.engine.embed(row_ptr, col_idx, d, **kw).items()}

    def heat(self, row_ptr, col_idx, d, **kw):
        return {k: v.cpu().numpy() for k, v in self.engine.heat(row_ptr, col_idx, d, **kw).items()}


def bound(fx):
    return R.VARIANT_FACTOR * fx["variant_distance"]


def check_parity(gw, name):
    fx = R.fixture(name)
    d, T = fx["d"], fx["d"] // 4
    out = gw.embed(fx["row_ptr"], fx["col_idx"], d)
    assert int(out["status"][0]) == 0
    chi = out["chi"]
    dist = float(np.abs(chi - fx["chi"]).max())
    rest = float(np.abs(chi - R.restatement(name)["chi"]).max())
    unit = fx["variant_distance"]
    print(f"graphwave parity {name}: max|chi - reference| {dist:.3g} = {dist / unit if unit else 0.0:.3g} x the variants' {unit:.3g}; "
          f"against the restatement {rest:.3g}")
    assert dist <= bound(fx) and rest <= bound(fx)
    assert np.array_equal(out["chi32"], chi.astype(np.float32))
    live = np.diff(fx["row_ptr"]) > 0
    assert not chi[~live].any() and not out["chi32"][~live].any()
    assert np.all(chi[live][:, [0, 2 * T]] == 1.0) and np.all(chi[live][:, [1, 2 * T + 1]] == 0.0)


def check_heat(gw, name):
    """one panel (the default width holds every column of these graphs) against the reference's ``heat_print``"""
    fx = R.fixture(name)
    n = fx["n_rows"]
    out = gw.heat(fx["row_ptr"], fx["col_idx"], fx["d"])
    assert int(out["status"][0]) == 0
    heat, ref = out["heat"], fx["heat_print"]
    assert heat.shape[2] >= n and not heat[:, :, n:].any()
    heat = heat[:, :, :n]
    assert np.array_equal(heat == 0, ref == 0)
    deg_max = int(np.diff(fx["row_ptr"]).max())
    for i, tau in enumerate(R.auto_taus(R.live_nodes(fx["row_ptr"]))):
        tol = (R.cheb_coefficients(tau).size) * (deg_max + 2) * EPS * float(np.abs(R.cheb_coefficients(tau)).sum())
        err = float(np.abs(heat[i] - ref[i]).max())
        print(f"graphwave heat {name} filter {i}: max error {err:.3g}, bound {tol:.3g}")
        assert err <= tol


def check_components(gw):
    """n257d64: ids 0..99 and 100..256 share no edge, so the heat between them is exactly zero before any threshold"""
    fx = R.fixture("n257d64")
    heat = gw.heat(fx["row_ptr"], fx["col_idx"], fx["d"])["heat"]
    assert not heat[:, :100, 100:257].any() and not heat[:, 100:, :100].any()
    assert heat[:, :100, :100].any() and heat[:, 100:, 100:257].any()


def check_bits(gw, name):
    """two calls give the same bits, and a panel of 64 columns the bits of the default panel"""
    fx = R.fixture(name)
    first = gw.embed(fx["row_ptr"], fx["col_idx"], fx["d"])
    assert gw.engine.panel_width(fx["n_rows"], fx["d"]) > 64 and gw.engine.panel_width(fx["n_rows"], fx["d"], 64) == 64
    for width in (0, 64):
        again = gw.embed(fx["row_ptr"], fx["col_idx"], fx["d"], width=width)
        assert int(first["status"][0]) == 0 and int(again["status"][0]) == 0
        for key in ("chi", "chi32"):
            assert np.array_equal(first[key], again[key]), (width, key)


def check_uniform_multiplicity(gw):
    """every entry of the multigraph twice: a uniform multiplicity cancels in M"""
    fx = R.fixture("multi130d32")
    assert (np.diff(fx["edges"], axis=0) == 0).all(axis=1).any()              # (the fixture itself lists edges twice)
    out = gw.embed(2 * fx["row_ptr"], np.repeat(fx["col_idx"], 2), fx["d"])
    assert int(out["status"][0]) == 0
    assert float(np.abs(out["chi"] - fx["chi"]).max()) <= bound(fx)


def check_status_bits(gw):
    fx = R.fixture("n40d4")
    rp, ci = fx["row_ptr"].astype(np.int64), fx["col_idx"]
    at = int(rp[np.argmax(np.diff(rp))])
    cases = {}
    cases["unsorted"] = ci.copy()
    cases["unsorted"][[at, at + 1]] = ci[[at + 1, at]]
    cases["range"] = ci.copy()
    cases["range"][5] = fx["n_rows"]
    cases["loop"] = ci.copy()
    row = int(np.searchsorted(rp, 5, side="right") - 1)
    cases["loop"][5] = row
    for what, bad in cases.items():
        res = gw.embed(fx["row_ptr"], bad, 8)
        assert int(res["status"][0]) & _cabi.STATUS_GRAPHWAVE_BAD_CSR, what
        assert np.isfinite(res["chi"]).all() and np.isfinite(res["chi32"]).all(), what
    assert not gw.embed(fx["row_ptr"], cases["range"], 8)["chi"].any()      # (the call ended where the entry was met)
    with pytest.raises(RuntimeError, match="not a sorted CSR"):
        gw.engine.check_status(gw.engine.embed(fx["row_ptr"], cases["range"], 8))


def check_refusals(gw):
    fx = R.fixture("n40d4")
    rp, ci = fx["row_ptr"], fx["col_idx"]
    with pytest.raises(RuntimeError, match="d 6 must be a multiple of 4"):
        gw.engine.embed(rp, ci, 6)
    with pytest.raises(RuntimeError, match="d 260.*GCC_GRAPHWAVE_MAX_DIM"):
        gw.engine.embed(rp, ci, 260)
    with pytest.raises(RuntimeError, match="width 96"):
        gw.engine.embed(rp, ci, 8, width=96)
    with pytest.raises(RuntimeError, match="n_rows 65537 outside"):
        gw.engine.embed(np.zeros(65538, dtype=np.int32), np.zeros(0, dtype=np.int32), 8)
    a, keep = gw.engine.graph_args(rp, ci, 8)
    status = torch.zeros(1, dtype=torch.int32, device=gw.device)
    chi = torch.zeros((fx["n_rows"], 8), dtype=torch.float64, device=gw.device)
    a.chi = gw.ptr(chi)
    with pytest.raises(RuntimeError, match="gcc_graphwave_embed.*chi32 is NULL"):
        gw.engine.call("gcc_graphwave_embed", a, status)
    with pytest.raises(RuntimeError, match="gcc_graphwave_heat.*heat is NULL"):
        gw.engine.call("gcc_graphwave_heat", a, status)
    a.chi32 = gw.ptr(torch.zeros((fx["n_rows"], 8), dtype=torch.float32, device=gw.device))
    with pytest.raises(RuntimeError, match="workspace_bytes 64 is less than gcc_graphwave_workspace_bytes"):
        gw.engine.call("gcc_graphwave_embed", a, status, workspace_bytes=64)
    a.row_ptr = None
    with pytest.raises(RuntimeError, match="row_ptr is NULL"):
        gw.engine.call("gcc_graphwave_embed", a, status)
    assert gw.lib.gcc_graphwave_workspace_bytes(40, 2 ** 31, 8, 0) < 0 and b"int32" in gw.lib.gcc_last_error()
    assert int(status.cpu()[0]) == 0 and not chi.cpu().numpy().any()        # (nothing was launched)


def check_cpu_tensor_refused(lib):
    fx = R.fixture("n40d4")
    eng = GraphWaveEngine(lib, _cabi.dev_ptr, "cpu")
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        eng.embed(fx["row_ptr"], fx["col_idx"], 8)
    assert ctypes.sizeof(_cabi.GccGraphwaveArgs) % 8 == 0
