"""The persistent fused update of linear layers (I2V_TUNE_FC_UPDATE = 1, fc_update_f32) against the tiled fused kernel
(I2V_TUNE_FC_UPDATE = 0) and against the separate filter gradient + SGD kernel: W' and m' bit for bit; and against the update
written out in float64 on the host, within a bound derived per element.

The library is imported inside the tests, as in the other GPU modules: collecting this file in a run without a GPU must not
load the HIP runtime into the process that runs the CPU tests."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, MOM, WD = 1e-2, 0.9, 5e-4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fused(x, gy, w, m, mode, hyper=None):
    from i2vsgg_amd._lib import TUNE, lib, ptr
    lr, mom, wd = hyper or (LR, MOM, WD)
    M, K = x.shape
    N = gy.shape[1]
    key = TUNE["I2V_FC_UPDATE"]
    saved = lib.i2v_get_tuning(key)
    assert lib.i2v_set_tuning(key, mode) == 0
    try:
        rc = lib.i2v_conv_wgrad_sgd(ptr(x), ptr(gy), ptr(w), ptr(m), M, 1, 1, K, N, 1, 1, 1, 0, lr, mom, wd, _stream())
    finally:
        lib.i2v_set_tuning(key, saved)
    assert rc == 0, lib.i2v_last_error().decode()


def _separate(x, gy, w, m, hyper=None):
    from i2vsgg_amd._lib import lib, ptr
    lr, mom, wd = hyper or (LR, MOM, WD)
    M, K = x.shape
    N = gy.shape[1]
    gw = torch.empty_like(w)
    # the gradient as ONE accumulator chain per output: left to itself the kernel splits the rows of a small filter (few
    # 64 x 64 tiles, many idle CUs) over several workgroups and adds their partial sums with atomics -- other roundings, and
    # bits that depend on arrival order.  The shapes of the first list have tiles enough and were never split; for the
    # 225 .. 257-row shapes of 1024 x 2048 the default would split in two, so there "separate" is the unsplit kernel, a
    # setting production does not use by default: a reference with one chain per output, not the shipped configuration.
    from i2vsgg_amd._lib import TUNE
    key = TUNE["I2V_WGRAD_PER_CU"]
    saved = lib.i2v_get_tuning(key)
    assert lib.i2v_set_tuning(key, 0) == 0
    try:
        rc = lib.i2v_conv_wgrad(ptr(x), ptr(gy), ptr(gw), M, 1, 1, K, N, 1, 1, 1, 0, 0.0, None, 0, _stream())
    finally:
        lib.i2v_set_tuning(key, saved)
    assert rc == 0, lib.i2v_last_error().decode()
    assert lib.i2v_sgd_momentum(ptr(w), ptr(gw), ptr(m), w.numel(), lr, mom, wd, _stream()) == 0


# (M rows, K taps, N filters): fc6, fc7, ragged rows, K not a multiple of the 64-tap tile, a column shard, rows past the
# register-resident limit (256: the tiled kernel takes over), and one stage past 128 rows (the 5-stage form)
SHAPES = [(128, 50176, 4096), (128, 4096, 4096), (22, 4096, 4096), (61, 9216, 4096), (64, 9216 + 4, 4096),
          (128, 9216, 512), (300, 4096, 4096), (160, 4096, 1024)]
IDS = ["fc6", "fc7", "m22", "m61", "k9220", "n512", "m300_fallback", "m160"]
# the stage counts the shapes above leave out (NS = ceil(M / 32) = 3, 6, 7, 8: own instantiations, own register and LDS
# budget), the last shape the kernel takes and the first it does not, and the masked edges: filter columns past N in the
# last strip (and a whole wave's), K of one tile, chunks of one tile (K / 64 tiles <= 256 / strips), more strips than CUs
# (one chunk), and 3 x 85 = 255 workgroups in a launch padded to 256 (the last one has nothing to do).  i2v_conv_wgrad_sgd
# itself refuses a filter of fewer than 512 tiles of 64 x 64 (its callers then take the separate kernels), so each shape is
# the smallest of its kind with ceil(N / 64) * ceil(K / 64) >= 512; REFUSED are shapes below that line
SHAPES += [(65, 1024, 2048), (96, 1024, 2048), (161, 1024, 2048), (192, 1024, 2048), (193, 1024, 2048), (224, 1024, 2048),
           (225, 1024, 2048), (256, 1024, 2048), (257, 1024, 2048), (128, 171 * 64 + 4, 132), (64, 32768, 4), (96, 4, 32768),
           (32, 64, 32896), (128, 5504, 384)]
IDS += ["m65_ns3", "m96_ns3", "m161_ns6", "m192_ns6", "m193_ns7", "m224_ns7", "m225_ns8", "m256_ns8", "m257_fallback",
        "n132_k10948", "n4", "k4", "strips257", "padded_launch"]
REFUSED = [(65, 1024, 256), (128, 1028, 132), (64, 256, 4), (96, 4, 128), (128, 5440, 384)]


def _entry_takes(M, K, N):
    """i2v_conv_wgrad_sgd's own condition: tiles enough to fill the chip without a split over rows."""
    return -(-N // 64) * -(-K // 64) >= 512 and M <= 4096


def _persistent(M, K, N):
    """launch_fc_update's conditions (csrc/wgrad.hip) for a linear problem the entry point takes: at most 256 rows, N and K
    multiples of 4, every operand below 2 GiB.  Returns the stage count NS it instantiates, or 0 for the tiled fallback."""
    assert _entry_takes(M, K, N)
    ok = M <= 256 and N % 4 == 0 and K % 4 == 0 and 4 * max(M * K, M * N, N * K) < 1 << 31
    return -(-M // 32) if ok else 0


def test_shapes_reach_every_stage_count():
    ns = dict((i, _persistent(*s)) for i, s in zip(IDS, SHAPES))
    assert set(ns.values()) == set(range(9))
    for i in IDS:
        if "_ns" in i:
            assert ns[i] == int(i[-1]), i
    assert ns["m257_fallback"] == 0 and ns["m300_fallback"] == 0
    cu, geom = 256, {}
    for i, (M, K, N) in zip(IDS, SHAPES):                # strips, chunks, tiles as launch_fc_update deals them
        strips, tiles = -(-N // 128), -(-K // 64)
        geom[i] = (strips, min(max(cu // strips, 1), tiles), tiles)
    assert geom["m65_ns3"] == (16, 16, 16) and geom["k4"] == (256, 1, 1)     # chunks == tiles: one tile per chunk
    assert geom["n132_k10948"] == (2, 128, 172) and geom["n4"] == (1, 256, 512)
    assert geom["strips257"][:2] == (257, 1)
    assert geom["padded_launch"] == (3, 85, 86) and (3 * 85) % 8 != 0
    assert not any(_entry_takes(*s) for s in REFUSED)


@pytest.mark.parametrize("mode", [1, 0])
def test_small_filters_are_refused_not_run(mode):
    """Below 512 tiles the entry point answers "unsupported" whichever fused kernel is selected, and touches nothing."""
    from i2vsgg_amd._lib import TUNE, lib, ptr
    key = TUNE["I2V_FC_UPDATE"]
    saved = lib.i2v_get_tuning(key)
    assert lib.i2v_set_tuning(key, mode) == 0
    try:
        for M, K, N in REFUSED:
            x, gy, w0, m0 = _inputs(M, K, N)
            w, m = w0.clone(), m0.clone()
            rc = lib.i2v_conv_wgrad_sgd(ptr(x), ptr(gy), ptr(w), ptr(m), M, 1, 1, K, N, 1, 1, 1, 0, LR, MOM, WD, _stream())
            torch.cuda.synchronize()
            assert rc != 0 and b"split over pixels" in lib.i2v_last_error()
            assert torch.equal(w, w0) and torch.equal(m, m0)
    finally:
        lib.i2v_set_tuning(key, saved)


def _inputs(M, K, N):
    g = torch.Generator(device=DEV).manual_seed(M * 7 + K + N)
    x = torch.randn(M, K, device=DEV, generator=g)
    gy = torch.randn(M, N, device=DEV, generator=g)
    w0 = torch.randn(N, K, device=DEV, generator=g) / 96
    m0 = torch.randn(N, K, device=DEV, generator=g) * 0.01
    return x, gy, w0, m0


def _run(name, x, gy, w0, m0, hyper=None):
    w, m = w0.clone(), m0.clone()
    if name == "separate":
        _separate(x, gy, w, m, hyper)
    else:
        _fused(x, gy, w, m, 1 if name == "new" else 0, hyper)
    torch.cuda.synchronize()
    return w, m


@pytest.mark.parametrize("M,K,N", SHAPES, ids=IDS)
def test_fc_update_bit_equal(M, K, N):
    x, gy, w0, m0 = _inputs(M, K, N)
    res = dict((name, _run(name, x, gy, w0, m0)) for name in ("new", "old", "separate"))
    for ref in ("old", "separate"):
        assert torch.equal(res["new"][0], res[ref][0]), "W' differs from the %s update" % ref
        assert torch.equal(res["new"][1], res[ref][1]), "m' differs from the %s update" % ref
    assert not torch.equal(res["new"][0], w0)


@pytest.mark.parametrize("M,K,N", SHAPES[1:], ids=IDS[1:])
def test_fc_update_against_float64(M, K, N):
    """Every shape but fc6 (its 128 x 50176 x 4096 host product is slow; fc7 runs the same code) against
        g = gy^T x,  m' = mom m + (g + wd w),  w' = w - lr m'
    in float64 on the host.  The bound is per element, with u = 2**-24 and S = |gy|^T |x|: a float32 sum of M products in
    any order is within (M + 4) u S of exact to first order (M - 1 additions and the products' own roundings -- the MFMA
    keeps them -- with room for the second-order terms); wd w, the sum g + wd w, mom m and the final sum round once each,
    every one an error of at most u times an operand that |mom m| + |wd w| + |g| bounds, 4 u of it in all.  w' adds the
    rounding of lr m' and of the difference, 2 u (|w| + lr |m'|), to lr times the error of m'."""
    from conftest import record_margin
    x, gy, w0, m0 = _inputs(M, K, N)
    w_dev, m_dev = (t.cpu().double() for t in _run("new", x, gy, w0, m0))
    x, gy, w, m = (t.cpu().double() for t in (x, gy, w0, m0))
    u = 2.0 ** -24
    g = gy.t() @ x
    e_m = (gy.abs().t() @ x.abs()).mul_((M + 4) * u)
    e_m += 4 * u * ((MOM * m).abs() + (WD * w).abs() + g.abs())
    m_ref = MOM * m + (g + WD * w)
    w_ref = w - LR * m_ref
    e_w = LR * e_m + 2 * u * (w.abs() + LR * m_ref.abs())
    assert (e_m > 0).all() and (e_w > 0).all()
    r_m = float(((m_dev - m_ref).abs() / e_m).max())
    r_w = float(((w_dev - w_ref).abs() / e_w).max())
    name = "test_fc_update_against_float64[%s]" % IDS[SHAPES.index((M, K, N))]
    record_margin(name, "|m' - float64| / E_m", r_m, 1.0)
    record_margin(name, "|w' - float64| / E_w", r_w, 1.0)
    assert r_m <= 1.0 and r_w <= 1.0


@pytest.mark.parametrize("hyper", [(LR, 0.0, 0.0), (LR, 0.9, 0.0)], ids=["plain_sgd", "no_decay"])
def test_fc_update_other_hyper_parameters(hyper):
    M, K, N = 96, 1024, 2048
    assert _persistent(M, K, N) == 3
    x, gy, w0, m0 = _inputs(M, K, N)
    new, sep = _run("new", x, gy, w0, m0, hyper), _run("separate", x, gy, w0, m0, hyper)
    assert torch.equal(new[0], sep[0]) and torch.equal(new[1], sep[1])
    assert not torch.equal(new[0], w0) and not torch.equal(new[1], m0)


def test_fc_update_default_on():
    from i2vsgg_amd._lib import TUNE, lib
    assert lib.i2v_get_tuning(TUNE["I2V_FC_UPDATE"]) == 1
