"""gcc_amd._engine.CabiEngine, the base of the downstream tasks' engines, without a GPU and without a library: the workspace is
reused and grows, the status word's bits are named, and only the product pointer function refuses a CPU tensor."""
import pytest
import torch

from gcc_amd import _cabi, logreg
from gcc_amd._engine import CabiEngine


def host_ptr(t):
    return 0 if t is None else t.data_ptr()


def test_workspace_grows_and_is_reused():
    eng = CabiEngine(lib=object(), ptr=host_ptr, device="cpu")
    first = eng.workspace(100)
    assert first.dtype == torch.uint8 and first.numel() == 256 and first.device.type == "cpu"
    assert eng.workspace(200) is first and eng.workspace(256, torch.device("cpu")) is first
    grown = eng.workspace(1000)
    assert grown is not first and grown.numel() == 1000
    assert eng.workspace(500) is grown and eng.workspace(1000) is grown


def test_raise_status_names_the_bits():
    bits = list(logreg.STATUS_BITS)
    texts = list(logreg.STATUS_BITS.values())
    clean = dict(status=torch.zeros(1, dtype=torch.int32))
    CabiEngine.raise_status(clean, "gcc_logreg", logreg.STATUS_BITS)
    one = dict(status=torch.tensor([bits[0]], dtype=torch.int32))
    with pytest.raises(RuntimeError) as e:
        CabiEngine.raise_status(one, "gcc_logreg", logreg.STATUS_BITS)
    assert str(e.value) == "gcc_logreg: " + texts[0]
    two = dict(status=torch.tensor([bits[0] | bits[2]], dtype=torch.int32))
    with pytest.raises(RuntimeError) as e:
        CabiEngine.raise_status(two, "gcc_logreg", logreg.STATUS_BITS)
    assert str(e.value) == "gcc_logreg: " + texts[0] + "; " + texts[2]
    with pytest.raises(RuntimeError) as e:
        CabiEngine.raise_status(two, "gcc_logreg", logreg.STATUS_BITS, allow=bits[0])
    assert str(e.value) == "gcc_logreg: " + texts[2]
    CabiEngine.raise_status(two, "gcc_logreg", logreg.STATUS_BITS, allow=bits[0] | bits[2])
    # the engines' own check_status goes through it, keyword and all
    capped = dict(status=torch.tensor([_cabi.STATUS_LR_ITER_CAP], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="^gcc_logreg: a problem stopped at the iteration cap"):
        logreg.LogRegEngine.check_status(capped)
    logreg.LogRegEngine.check_status(capped, allow_iter_cap=True)


def test_a_cpu_tensor_is_refused_by_the_product_pointer_alone():
    emb = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    product = CabiEngine(lib=object())
    assert product.ptr is _cabi.dev_ptr
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        product.require_device(emb)
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        product.table(emb)
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        product.require_device(torch.device("cpu"))
    injected = CabiEngine(lib=object(), ptr=host_ptr)
    injected.require_device(emb)
    assert injected.table(emb) == (emb.data_ptr(), 3, 4, 4)
    assert injected.table(emb[:, :3], "emb_q") == (emb.data_ptr(), 3, 3, 4)      # a row stride larger than D is served
    assert injected.table(emb[:1]) == (emb.data_ptr(), 1, 4, 4)
    with pytest.raises(ValueError, match="^emb_q must be a float32 matrix with unit stride along its rows$"):
        injected.table(emb.t(), "emb_q")
    with pytest.raises(ValueError, match="^emb must be a float32 matrix"):
        injected.table(emb.double())
