"""i2v_epilogue_bwd called on its own, with ordered column sums (I2V_TUNE_SPLIT_ATOMICS = 0) through the current context's
split workspace: g_pre = gy * (y > 0), g = g_pre * scale[n], g_t = g column-major, gbias[n] += sum_m g_pre[m][n].

The kernels live in csrc/elementwise.hip; the reduce pass behind the N % 4 != 0 form is a kernel of csrc/wgrad.hip reached
through a host function, which only whole training steps covered before.  The shapes are the smallest that reach each kernel
and each finish of the column sums (host logic of i2v_epilogue_bwd):

  10 x 18      N % 4 != 0: epilogue_bwd_scalar_kernel on 3 row blocks of 4 rows (the last has 2) + the scalar reduce pass
  10 x 8       epilogue_bwd_kernel, 3 row blocks, one-level finish
  2052 x 1024  epilogue_bwd_kernel, more than 2^21 elements: 513 row blocks of 4 rows in 17 groups of 32, two-level finish
  1030 x 8     epilogue_bwd_narrow_kernel (N <= 512, M >= 1024, no g_t): 128 row lanes, 9 row blocks of 128 rows
  1030 x 16    the same with 64 row lanes: 17 row blocks of 64 rows

g, g_pre and g_t are one select and one multiply per element (the library is built with -ffp-contract=off), so they equal
torch's fp32 expression bit for bit.  gbias is compared with the float64 column sum of g_pre within M * 2^-24 * sum|g_pre|
per column, which bounds the error of an fp32 sum of M terms in ANY order (each of at most M - 1 additions rounds by at most
2^-24 of a partial sum, and no partial sum exceeds sum|g_pre| by more than that factor); two calls must agree bit for bit.

The library is imported inside the tests, as in the other GPU modules."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (M, N, with g_t)
CASES = [(10, 18, False), (10, 18, True), (10, 8, True), (2052, 1024, False), (1030, 8, False), (1030, 16, False)]
IDS = ["scalar_reduce", "scalar_reduce_gt", "vector_one_level", "vector_two_levels", "narrow", "narrow_17_blocks"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(gy, y, scale, relu, want_gt):
    from i2vsgg_amd import ops
    M, N = gy.shape
    g, gpre = torch.empty_like(gy), torch.empty_like(gy)
    g_t = torch.empty((N, M), device=gy.device, dtype=torch.float32) if want_gt else None
    gbias = torch.zeros((N,), device=gy.device, dtype=torch.float32)
    rc = ops.lib.i2v_epilogue_bwd(ops.ptr(gy), ops.ptr(y) if relu else None, ops.ptr(scale), ops.ptr(g), ops.ptr(gpre),
                                  ops.ptr(gbias), M, N, int(relu), ops.ptr(g_t), *ops.launch.split_args(gy.device), ops.stream())
    assert rc == 0, ops.lib.i2v_last_error().decode()
    return g, gpre, g_t, gbias


@pytest.mark.parametrize("relu_scale", [True, False], ids=["relu_scale", "plain"])
@pytest.mark.parametrize("M,N,want_gt", CASES, ids=IDS)
def test_epilogue_bwd_ordered(M, N, want_gt, relu_scale):
    from i2vsgg_amd._lib import TUNE, lib
    gen = torch.Generator().manual_seed(1000 * M + N)
    gy = torch.randn((M, N), generator=gen).to(DEV)
    y = torch.randn((M, N), generator=gen).to(DEV)
    scale = (torch.randn((N,), generator=gen) + 1.5).to(DEV) if relu_scale else None

    key = TUNE["I2V_SPLIT_ATOMICS"]
    saved = lib.i2v_get_tuning(key)
    assert lib.i2v_set_tuning(key, 0) == 0
    lib.i2v_ordered_fallbacks(1)
    try:
        g, gpre, g_t, gbias = _run(gy, y, scale, relu_scale, want_gt)
        again = _run(gy, y, scale, relu_scale, want_gt)[3]
    finally:
        lib.i2v_set_tuning(key, saved)
    torch.cuda.synchronize()
    assert lib.i2v_ordered_fallbacks(1) == 0

    want_pre = torch.where(y > 0, gy, torch.zeros_like(gy)) if relu_scale else gy
    want_g = want_pre * scale[None, :] if relu_scale else want_pre
    assert torch.equal(_bits(gpre), _bits(want_pre))
    assert torch.equal(_bits(g), _bits(want_g))
    if want_gt:
        assert torch.equal(_bits(g_t), _bits(want_g.t()))

    col = want_pre.double().sum(0)
    bound = M * 2.0 ** -24 * want_pre.double().abs().sum(0)
    err = (gbias.double() - col).abs()
    print("epilogue_bwd %d x %d: max |gbias - sum64| / bound = %.3g" % (M, N, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    assert torch.equal(_bits(gbias), _bits(again))
