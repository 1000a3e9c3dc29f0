"""GPU parity tests of the HBM-bound "glue" kernels (clipa_amd/csrc/misc.hip) and of the optimizer / gradient-exchange
kernels (clipa_amd/csrc/runtime.hip) at production shapes and at the edges of their launch geometry, through
clipa_amd.ops.  The cases, their inputs (exact-sum data for reductions, position-coded data for data movement), the
references and the comparisons live in tests/glue_cases.py; every comparison there is torch.equal except where the
device's own sqrt / division enters.  Each test is parametrised by case name, so a failure names its branch.
"""
import pytest
import torch

from . import glue_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from clipa_amd import ops as _ops
    return _ops


def query(name, *args):
    from clipa_amd import lib
    return lib.query(name, *args)


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", G.ASSEMBLE, ids=G.names(G.ASSEMBLE))
def test_assemble_tokens(case):
    G.check_assemble_tokens(ops(), DEV, case)


@pytest.mark.parametrize("case", G.ASSEMBLE_BWD, ids=G.names(G.ASSEMBLE_BWD))
def test_assemble_tokens_bwd(case):
    G.check_assemble_tokens_bwd(ops(), DEV, case, query)


@pytest.mark.parametrize("case", G.EMBED, ids=G.names(G.EMBED))
def test_embed_tokens(case):
    G.check_embed_tokens(ops(), DEV, case)


@pytest.mark.parametrize("case", G.EMBED_BWD, ids=G.names(G.EMBED_BWD))
def test_embed_tokens_bwd(case):
    G.check_embed_tokens_bwd(ops(), DEV, case, query)


@pytest.mark.parametrize("case", G.ARGMAX, ids=G.names(G.ARGMAX))
def test_argmax_tokens(case):
    G.check_argmax_tokens(ops(), DEV, case)


@pytest.mark.parametrize("case", G.POOL, ids=G.names(G.POOL))
def test_pool_fwd_bwd(case):
    G.check_pool(ops(), DEV, case)


@pytest.mark.parametrize("case", G.ROWS, ids=G.names(G.ROWS))
def test_gather_scatter_rows(case):
    G.check_rows(ops(), DEV, case)


@pytest.mark.parametrize("case", G.L2NORM, ids=G.names(G.L2NORM))
def test_l2norm_fwd_bwd(case):
    G.check_l2norm(ops(), DEV, case)


@pytest.mark.parametrize("case", G.COLSUM, ids=G.names(G.COLSUM))
def test_colsum(case):
    G.check_colsum(ops(), DEV, case, query)


@pytest.mark.parametrize("case", G.CAST, ids=G.names(G.CAST))
def test_casts(case):
    G.check_cast(ops(), DEV, case)


@pytest.mark.parametrize("case", G.TRANSPOSE, ids=G.names(G.TRANSPOSE))
def test_transpose_bf16(case):
    G.check_transpose(ops(), DEV, case)


@pytest.mark.parametrize("case", G.SUM_SCALE, ids=G.names(G.SUM_SCALE))
def test_sum_scale(case):
    G.check_sum_scale(ops(), DEV, case)


@pytest.mark.parametrize("case", G.REDUCE_SMALL + G.REDUCE_BIG, ids=G.names(G.REDUCE_SMALL + G.REDUCE_BIG))
def test_reduce_shards(case):
    G.check_reduce_shards(ops(), DEV, case)


def test_reduce_shards_rejects_ragged_sizes():
    G.check_reduce_shards_errors(ops(), DEV)


@pytest.mark.parametrize("case", G.ADAMW, ids=G.names(G.ADAMW))
def test_adamw(case):
    G.check_adamw(ops(), DEV, case)


@pytest.mark.parametrize("case", G.ADAMW_MULTI, ids=G.names(G.ADAMW_MULTI))
def test_adamw_multi(case):
    G.check_adamw_multi(ops(), DEV, case)


@pytest.mark.parametrize("case", G.SQNORM, ids=G.names(G.SQNORM))
def test_grad_sqnorm(case):
    G.check_grad_sqnorm(ops(), DEV, case)


@pytest.mark.parametrize("case", G.CLIP_COEF, ids=G.names(G.CLIP_COEF))
def test_clip_coef(case):
    G.check_clip_coef(ops(), DEV, case)


def test_grad_clip_coef_non_finite_gradient():
    G.check_grad_clip_coef_nonfinite(ops(), DEV)
