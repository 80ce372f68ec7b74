"""The ProNE kernels (gcc_amd/csrc/prone.hip) on a real MI355X against the reference's own runs, scipy and NumPy: the checks of
tests/prone_check.py on every fixture, the wide ones (d = 64, k = 74: two columns per lane, the eigensolver's 74 x 74 problem,
the square Q) included."""
import pytest

from tests import prone_check as C
from tests import prone_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pr():
    from gcc_amd import _cabi

    return C.Pr(_cabi.load(), _cabi.dev_ptr, "cuda:0")


@pytest.mark.parametrize("name", R.FIXTURES)
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


@pytest.mark.parametrize("n,k", [(201, 26), (300, 12), (75, 16), (1100, 26), (74, 74), (1100, 74)])
def test_orthonormalisation(pr, n, k):
    C.check_orthonormalize(pr, n, k, seed=n + k)


@pytest.mark.parametrize("name,chunks", [("hub", (0, 32, C.SPLIT_CHUNK)), ("n120d64", (0, 2048))])
def test_two_calls_and_every_chunk_give_the_same_bits(pr, name, chunks):
    C.check_bits(pr, name, chunks)


def test_device_graph_is_served_and_a_multigraph_parent_refused(pr):
    C.check_device_graph(pr)


def test_each_status_bit(pr):
    C.check_status_bits(pr)


def test_limits_short_workspace_and_null_members_are_refused_by_name(pr):
    C.check_refusals(pr)


def test_cpu_tensor_is_refused(pr):
    C.check_cpu_tensor_refused(pr.lib)
