"""The persistent fused update of linear layers (I2V_TUNE_FC_UPDATE = 1, fc_update_f32) against the tiled fused kernel
(I2V_TUNE_FC_UPDATE = 0) and against the separate filter gradient + SGD kernel: W' and m' bit for bit.

The library is imported inside the tests, as in the other GPU modules: collecting this file in a run without a GPU must not
load the HIP runtime into the process that runs the CPU tests."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, MOM, WD = 1e-2, 0.9, 5e-4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fused(x, gy, w, m, mode):
    from i2vsgg_amd._lib import TUNE, lib, ptr
    M, K = x.shape
    N = gy.shape[1]
    key = TUNE["I2V_FC_UPDATE"]
    saved = lib.i2v_get_tuning(key)
    assert lib.i2v_set_tuning(key, mode) == 0
    try:
        rc = lib.i2v_conv_wgrad_sgd(ptr(x), ptr(gy), ptr(w), ptr(m), M, 1, 1, K, N, 1, 1, 1, 0, LR, MOM, WD, _stream())
    finally:
        lib.i2v_set_tuning(key, saved)
    assert rc == 0, lib.i2v_last_error().decode()


def _separate(x, gy, w, m):
    from i2vsgg_amd._lib import lib, ptr
    M, K = x.shape
    N = gy.shape[1]
    gw = torch.empty_like(w)
    assert lib.i2v_conv_wgrad(ptr(x), ptr(gy), ptr(gw), M, 1, 1, K, N, 1, 1, 1, 0, 0.0, None, 0, _stream()) == 0
    assert lib.i2v_sgd_momentum(ptr(w), ptr(gw), ptr(m), w.numel(), LR, MOM, WD, _stream()) == 0


# (M rows, K taps, N filters): fc6, fc7, ragged rows, K not a multiple of the 64-tap tile, a column shard, rows past the
# register-resident limit (256: the tiled kernel takes over), and one stage past 128 rows (the 5-stage form)
SHAPES = [(128, 50176, 4096), (128, 4096, 4096), (22, 4096, 4096), (61, 9216, 4096), (64, 9216 + 4, 4096),
          (128, 9216, 512), (300, 4096, 4096), (160, 4096, 1024)]


@pytest.mark.parametrize("M,K,N", SHAPES, ids=["fc6", "fc7", "m22", "m61", "k9220", "n512", "m300_fallback", "m160"])
def test_fc_update_bit_equal(M, K, N):
    g = torch.Generator(device=DEV).manual_seed(M * 7 + K + N)
    x = torch.randn(M, K, device=DEV, generator=g)
    gy = torch.randn(M, N, device=DEV, generator=g)
    w0 = torch.randn(N, K, device=DEV, generator=g) / 96
    m0 = torch.randn(N, K, device=DEV, generator=g) * 0.01
    res = {}
    for name in ("new", "old", "separate"):
        w, m = w0.clone(), m0.clone()
        if name == "separate":
            _separate(x, gy, w, m)
        else:
            _fused(x, gy, w, m, 1 if name == "new" else 0)
        torch.cuda.synchronize()
        res[name] = (w, m)
    for ref in ("old", "separate"):
        assert torch.equal(res["new"][0], res[ref][0]), "W' differs from the %s update" % ref
        assert torch.equal(res["new"][1], res[ref][1]), "m' differs from the %s update" % ref
    assert not torch.equal(res["new"][0], w0)


def test_fc_update_default_on():
    from i2vsgg_amd._lib import TUNE, lib
    assert lib.i2v_get_tuning(TUNE["I2V_FC_UPDATE"]) == 1
