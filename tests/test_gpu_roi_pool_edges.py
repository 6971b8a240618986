"""Caffe ROIPool on the device (i2v_roi_pool_fwd, i2v_roi_pool_fwd_geom, i2v_roi_pool_bwd: roi_pool_fwd_c128_kernel,
roi_pool_fwd_kernel and roi_pool_bwd_kernel of csrc/roi_ops.hip) against the numpy reference of tests/roi_pool_ref.py, on the maps
and ROIs where its decisions are close: tied maxima (first cell in (h, w) order wins), all-negative windows whose cell count is no
multiple of the eight cells fetched at a time, extents at which the float32 bin rule reaches a cell further than the integer one,
corners on the half, ROIs over and beyond every border, -FLT_MAX / -inf / NaN planes.  Values and argmax are exact: no tolerance.
The reference itself is held to the C oracle and to torch's adaptive max pool in tests/test_roi_pool_ref_host.py.
Needs a real MI355X: `pytest -m gpu`."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import roi_pool_ref as rp

from conftest import record_margin

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CMAX = 256
# 128: one chunk of the c128 kernel; 256: two (c0 > 0); 100: the generic kernel, 64 + a ragged 36; 4
CHANNELS = (128, 256, 100, 4)
BWD_MAPS = ("constant", "tied", "specials")
BWD_GRIDS = ((7, 7), (3, 5))
_ids = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from i2vsgg_amd import ops as o
    return o


@contextlib.contextmanager
def c128_route(on):
    """I2V_ROIPOOL_C128: 1 = the default (NHWC maps with C % 128 == 0 and P <= 64 take roi_pool_fwd_c128_kernel), 0 = the generic kernel."""
    from i2vsgg_amd._lib import TUNE, lib
    assert lib.i2v_get_tuning(TUNE["I2V_ROIPOOL_C128"]) == 1
    try:
        assert lib.i2v_set_tuning(TUNE["I2V_ROIPOOL_C128"], on) == 0
        yield
    finally:
        lib.i2v_set_tuning(TUNE["I2V_ROIPOOL_C128"], 1)
    assert lib.i2v_get_tuning(TUNE["I2V_ROIPOOL_C128"]) == 1


@functools.lru_cache(maxsize=None)
def _map(name, shape):
    """The map at the widest C; channel c is the same at every narrower C."""
    f = rp.make_map(name, shape[0], CMAX, shape[1], shape[2])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _windows(name, shape):
    return {}


def _reference(name, shape, grid):
    """ROIs, values and argmax at CMAX channels; every distinct window of a map is walked once for all grids."""
    rois = rp.all_rois(*shape, *grid)
    out, arg = rp.roi_pool_fwd(_map(name, shape), rois, grid[0], grid[1], rp.SCALE, windows=_windows(name, shape))
    return rois, out, arg


def _feat(name, shape, C, nhwc):
    f = torch.from_numpy(_map(name, shape)[:, :C].copy()).to(DEV)
    return f.contiguous(memory_format=torch.channels_last) if nhwc else f


def _routes(C, nhwc):
    return (1, 0) if (nhwc and C % 128 == 0) else (1,)


def _same_bits(got, want, what):
    """got: a device tensor in either memory format; want: a device tensor of the same logical shape."""
    assert got.shape == want.shape, what
    if got.dtype == torch.float32:
        got, want = got.view(torch.int32), want.view(torch.int32)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        at = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d differ, first at (r, c, ph, pw) = %s: got %s, want %s"
                             % (what, bad.shape[0], got.numel(), at, got[at].item(), want[at].item()))


@pytest.mark.parametrize("name", rp.MAP_NAMES)
@pytest.mark.parametrize("shape", rp.MAP_SHAPES, **_ids)
@pytest.mark.parametrize("grid", rp.GRIDS, **_ids)
def test_forward_values_and_argmax_are_the_reference_bit_for_bit(ops, grid, shape, name):
    """Every ROI set in one launch, at every channel count, map layout, output layout and route."""
    rois, out, arg = _reference(name, shape, grid)
    rd = torch.from_numpy(rois).to(DEV)
    want_o, want_a = torch.from_numpy(out).to(DEV), torch.from_numpy(arg).to(DEV)
    for C in CHANNELS:
        wo, wa = want_o[:, :C], want_a[:, :C]
        for nhwc in (True, False):
            f = _feat(name, shape, C, nhwc)
            for on in _routes(C, nhwc):
                with c128_route(on):
                    for out_nchw in (True, False):
                        what = (C, "nhwc" if nhwc else "nchw", "out_nchw" if out_nchw else "out_nhwc", on)
                        o, a = ops.roi_pool(f, rd, grid[0], grid[1], rp.SCALE, out_nchw=out_nchw, return_argmax=True)
                        assert o.is_contiguous(memory_format=torch.contiguous_format if out_nchw else torch.channels_last)
                        _same_bits(o, wo, ("values",) + what)
                        _same_bits(a, wa, ("argmax",) + what)


@pytest.mark.parametrize("name", rp.MAP_NAMES)
@pytest.mark.parametrize("shape", rp.MAP_SHAPES, **_ids)
@pytest.mark.parametrize("grid", rp.GRIDS, **_ids)
def test_packed_maps_equal_the_static_call(ops, grid, shape, name):
    """The maps at the start of a larger buffer whose extent the kernel reads from device memory; the rest of the buffer holds
    +1e30, which would win any maximum it leaked into."""
    B, H, W = shape
    geom = torch.tensor([H, W], dtype=torch.int32, device=DEV)
    rois, out, _ = _reference(name, shape, grid)
    rd = torch.from_numpy(rois).to(DEV)
    want_o = torch.from_numpy(out).to(DEV)
    for C in CHANNELS:
        f = _feat(name, shape, C, True)
        cap = H * W + 13
        buf = torch.full((B * cap * C,), 1e30, dtype=torch.float32, device=DEV)
        buf[:B * H * W * C] = f.permute(0, 2, 3, 1).reshape(-1)
        maps = ops.PackedMaps(buf, B, C, geom)
        assert maps.cap_cells == cap
        _same_bits(maps.view(H, W), f, "the packed maps")
        for on in _routes(C, True):
            with c128_route(on):
                for out_nchw in (True, False):
                    what = (C, "out_nchw" if out_nchw else "out_nhwc", on)
                    got = ops.roi_pool_packed(maps, rd, grid[0], grid[1], rp.SCALE, out_nchw=out_nchw)
                    static = ops.roi_pool(f, rd, grid[0], grid[1], rp.SCALE, out_nchw=out_nchw)
                    _same_bits(got, static, ("packed vs static",) + what)
                    _same_bits(got, want_o[:, :C], ("packed vs reference",) + what)


def test_grid_past_the_lds_stage_is_refused_by_the_status_word(ops):
    """PH * PW <= 256 is the limit: 16 x 16 runs (above), 17 x 16 comes back as a status, before any launch, on both entry points."""
    from i2vsgg_amd._lib import I2VError
    shape = rp.MAP_SHAPES[0]
    f = _feat("tied", shape, 128, True)
    rd = torch.from_numpy(rp.all_rois(*shape, 7, 7)).to(DEV)
    for ph, pw in ((17, 16), (16, 17), (1, 257)):
        with pytest.raises(I2VError, match="pooled grid too large"):
            ops.roi_pool(f, rd, ph, pw, rp.SCALE)
        maps = ops.PackedMaps(f.permute(0, 2, 3, 1).reshape(-1).clone(), shape[0], 128, torch.tensor(shape[1:], dtype=torch.int32, device=DEV))
        with pytest.raises(I2VError, match="pooled grid too large"):
            ops.roi_pool_packed(maps, rd, ph, pw, rp.SCALE)
    torch.cuda.synchronize()
    assert ops.roi_pool(f, rd, 1, 256, rp.SCALE).shape == (rd.shape[0], 128, 1, 256)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", rp.MAP_SHAPES, **_ids)
def test_two_forward_runs_give_the_same_bits(ops, shape):
    rd = torch.from_numpy(rp.all_rois(*shape, 7, 7)).to(DEV)
    for name in ("tied", "specials"):
        for C in (256, 100):
            f = _feat(name, shape, C, True)
            for on in _routes(C, True):
                with c128_route(on):
                    o1, a1 = ops.roi_pool(f, rd, 7, 7, rp.SCALE, return_argmax=True)
                    o2, a2 = ops.roi_pool(f, rd, 7, 7, rp.SCALE, return_argmax=True)
                    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(a1, a2), (name, C, on)


@pytest.mark.parametrize("grid", BWD_GRIDS, **_ids)
@pytest.mark.parametrize("shape", rp.MAP_SHAPES, **_ids)
@pytest.mark.parametrize("name", BWD_MAPS)
def test_backward_is_the_float64_scatter_within_the_summation_bound(ops, name, shape, grid):
    """Maps on which many bins and many ROIs send their gradient to one cell.  The kernel adds float32 terms in no fixed order: per
    map cell |got - ref| <= n * 2^-24 * sum |g| with n terms (the bound of a float32 sum of n terms in any order); a cell with no
    term is exactly zero -- every cell of the -FLT_MAX, -inf and NaN planes among them -- and a cell with one term is exact.
    The ROI sets without `sizes`: overlapping ROIs are what piles gradients up, not the walk's length."""
    rois = np.concatenate([r for key, r in rp.roi_sets(*shape, *grid).items() if key != "sizes"])
    out, arg = rp.roi_pool_fwd(_map(name, shape), rois, grid[0], grid[1], rp.SCALE, windows=_windows(name, shape))
    gout = np.random.default_rng(17).standard_normal(out.shape, dtype=np.float32)
    gin, n, sabs = rp.roi_pool_bwd(gout, rois, arg, _map(name, shape).shape)
    assert n.max() > 8 and (n == 1).any() and (n == 0).any()
    if name == "specials":
        assert not n[:, [0, 1, 3]].any() and n[:, 2].any()
    bound = rp.bwd_bound(n, sabs)
    rd = torch.from_numpy(rois).to(DEV)
    worst = 0.0
    for C in CHANNELS:
        g = torch.from_numpy(gout[:, :C].copy()).to(DEV)
        want_a = torch.from_numpy(arg[:, :C].copy()).to(DEV)
        nn, bb = n[:, :C], bound[:, :C]
        many = nn > 1
        for nhwc in (True, False):
            for out_nchw in (True, False):
                what = (C, nhwc, out_nchw)
                ft = torch.from_numpy(_map(name, shape)[:, :C].copy()).to(DEV).requires_grad_()
                f = ft.contiguous(memory_format=torch.channels_last) if nhwc else ft
                o, a = ops.roi_pool(f, rd, grid[0], grid[1], rp.SCALE, out_nchw=out_nchw, return_argmax=True)
                _same_bits(a, want_a, ("argmax",) + what)
                o.backward(g)
                got = ft.grad.cpu().numpy().astype(np.float64)
                err = np.abs(got - gin[:, :C])
                assert np.all(got[nn == 0] == 0), what
                assert np.all(err[nn == 1] == 0), what
                ratio = float((err[many] / bb[many]).max())
                worst = max(worst, ratio)
                assert np.all(err <= bb), (what, ratio)
    record_margin("test_backward_is_the_float64_scatter[%s-%s-%s]" % (name, "x".join(map(str, shape)), "x".join(map(str, grid))),
                  "max |got - ref| / (n 2^-24 sum|g|)", worst, 1.0)
