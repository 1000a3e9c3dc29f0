"""The case table of tests/glue_cases.py through tests/cpu_ops - the torch stand-ins that the 2- and 8-rank gloo tests and
the engine CPU tests stand on - so that the stand-ins keep the contracts the kernels are held to in
tests/test_glue_kernels_gpu.py: rows outside [0, n), zero rows, the clamp slot, the NaN coefficient, `accumulate`,
saturation and NaN rows of the embedding gradient.  It also lets the case table and its references be debugged without a
GPU.  The comparisons are the GPU file's: the exact-sum and position-coded cases are exact for any correct
implementation and the tolerances (l2norm, clip_coef, AdamW) are the same ones.  This is not an independent check
everywhere: the embed_tokens_bwd, reduce_shards, pool and l2norm stand-ins are written to the kernels' arithmetic and so
restate the case references; for those ops this file only pins the stand-in to the contract, so that it cannot drift
from what the device test holds the kernel to.
"""
import pytest

from . import cpu_ops
from . import glue_cases as G

DEV = "cpu"
query = None


def ops():
    return cpu_ops


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
