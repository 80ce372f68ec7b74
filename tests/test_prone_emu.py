"""The ProNE kernels (gcc_amd/csrc/prone.hip) on the lock-step emulator against the reference's own runs, scipy and NumPy: the
checks of tests/prone_check.py on the fixtures of n <= 300 and d <= 16.  The wide fixtures run on the GPU only."""
import pytest

from tests import prone_check as C
from tests import prone_reference as R
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_logreg import emu_ptr


@pytest.fixture(scope="module")
def pr():
    return C.Pr(emu_lib(), emu_ptr, "cpu")


@pytest.mark.parametrize("name", R.EMU_FIXTURES)
def test_embedding_is_the_references(pr, name):
    C.check_parity(pr, name)


def test_step_one_returns_the_factorisation(pr):
    C.check_step_one(pr)


@pytest.mark.parametrize("name", ["hub", "n40d2"])
def test_node_terms_agree_with_numpy(pr, name):
    C.check_node_terms(pr, name)


@pytest.mark.parametrize("name,k,chunk", [("hub", 12, C.SPLIT_CHUNK), ("hub", 16, C.SPLIT_CHUNK), ("hub", 26, 32), ("hub", 74, C.SPLIT_CHUNK),
                                          ("n201d16", 74, 0), ("n201d16", 26, 0)])
def test_every_product_and_tail_agrees_with_scipy(pr, name, k, chunk):
    C.check_spmm(pr, name, k, chunk)


@pytest.mark.parametrize("n,k", [(201, 26), (300, 12), (75, 16), (1100, 26)])
def test_orthonormalisation(pr, n, k):
    C.check_orthonormalize(pr, n, k, seed=n + k)


def test_two_calls_and_every_chunk_give_the_same_bits(pr):
    C.check_bits(pr, "hub")


def test_device_graph_is_served_and_a_multigraph_parent_refused(pr):
    C.check_device_graph(pr)


def test_each_status_bit(pr):
    C.check_status_bits(pr)


def test_limits_short_workspace_and_null_members_are_refused_by_name(pr):
    C.check_refusals(pr)


def test_product_path_refuses_cpu_tensors():
    C.check_cpu_tensor_refused(emu_lib())


@pytest.mark.parametrize("name", R.FIXTURES)
def test_numpy_restatement_is_pinned_to_the_fixtures(name):
    fx = R.fixture(name)
    emb = R.embed_numpy(fx["row_ptr"], fx["col_idx"], fx["d"], omega=fx["omega"])["emb"]
    assert float(abs(R.align(emb, fx["emb_lu"]) - fx["emb_lu"]).max()) <= R.VARIANT_FACTOR * fx["variant_distance"]
    assert not emb[(fx["row_ptr"][1:] - fx["row_ptr"][:-1]) == 0].any()


def test_bessel_series_is_scipys():
    from scipy.special import iv

    for order in range(8):
        for x in (0.1, 0.5, 2.0):
            assert abs(R.bessel_iv(order, x) - iv(order, x)) <= 4 * 2.0 ** -52 * iv(order, x)
