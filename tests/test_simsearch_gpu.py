"""gcc_sim_search on a real MI355X against the float64 restatement of tests/simsearch_check.py: the checks of the emulator
tier, then many workgroups with merged splits, and a side stream with a reused workspace."""
import numpy as np
import pytest
import torch

from tests import simsearch_check as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sim():
    from gcc_amd import _cabi

    return C.Sim(_cabi.load(), _cabi.dev_ptr, "cuda:0")


@pytest.mark.parametrize("tier", ["exact", "norm"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_search_equals_the_restatement(sim, name, tier):
    C.check_case(sim, name, tier)


def test_duplicate_rows_tie_bitwise_and_list_in_column_order(sim):
    C.check_duplicate_rows(sim)


def test_zero_row_sets_its_status_bit_and_scores_zero(sim):
    C.check_zero_row(sim)


def test_out_of_range_index_is_absent_with_a_status_bit(sim):
    C.check_bad_index(sim)


def test_bad_arguments_are_refused_by_name_with_nothing_written(sim):
    C.check_refusals(sim)


def test_engine_recall_and_argument_errors(sim):
    C.check_engine(sim)


@pytest.fixture(scope="module")
def large():
    """exact tier at (4096, 8192, 64), k = 40: 64 query tiles, and the float64 restatement by one matmul and one stable sort"""
    rng = np.random.RandomState(5)
    mq, mc, D, k = 4096, 8192, 64, 40
    emb_q = rng.randint(-3, 4, (mq, D)).astype(np.float32)
    emb_c = rng.randint(-3, 4, (mc, D)).astype(np.float32)
    target = rng.randint(0, mc, mq).astype(np.int32)
    target[::7] = -1
    s = emb_q.astype(np.float64) @ emb_c.astype(np.float64).T
    st = s[np.arange(mq), np.maximum(target, 0)][:, None]
    have = target >= 0
    ref = dict(greater=np.where(have, (s > st).sum(1), -1).astype(np.int32),
               equal_before=np.where(have, ((s == st) & (np.arange(mc)[None, :] < target[:, None])).sum(1), -1).astype(np.int32),
               target_score=np.where(have, st[:, 0], np.nan))
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]         # stable: equal scores keep their column order
    ref["topk_col"] = order.astype(np.int32)
    ref["topk_score"] = np.take_along_axis(s, order, 1)
    ref["target"] = np.where(have, target, -1)
    return dict(emb_q=emb_q, emb_c=emb_c, q_idx=None, c_idx=None, target=target, k=k, ld_extra=0, normalize=0, ref=ref)


@pytest.mark.parametrize("splits", [0, 5])
def test_many_workgroups_and_merged_splits_exactly(sim, large, splits):
    got = sim.search(dict(large, splits=splits))
    assert got["status"][0] == 0
    C.assert_exact(got, large["ref"])
    C.assert_hits_agree(got, large["ref"])


def test_side_stream_and_reused_workspace_give_the_same_results(sim):
    p, p2 = C.problem("130x1000", "norm"), C.problem("130x1000s3", "norm")
    first, first2 = sim.search(p), sim.search(p2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = sim.search(p)
        again2 = sim.search(p2)                                  # the same engine: the second call reuses the workspace
    side.synchronize()
    for a, b in ((first, again), (first2, again2)):
        for key in ("greater", "equal_before", "topk_col", "status"):
            assert np.array_equal(a[key], b[key]), key
        for key in ("target_score", "topk_score"):
            assert np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), key
