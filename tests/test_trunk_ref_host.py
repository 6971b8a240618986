"""The masked float64 reference of the trunk (tests/trunk_ref.py) checked on its own, on the CPU: against a plainly written
F.relu / F.conv2d / F.max_pool2d network, against its own float32 run under shared masks (the e32 that sets the bounds of
tests/test_gpu_trunk.py), and against every planted wiring error -- each must move a compared tensor by 10 x the bound in force for
that tensor, which is what gives the GPU test teeth.  And the reference of the stem's max pool (indices and backward of
F.max_pool2d in float64) against three plain loops, on inputs full of ties."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bottleneck_ref as B
import trunk_ref as R
from conftest import record_margin

SHARED_MASK_BOUND = 1e-5        # the float32 run against the float64 run under the same masks: rounding, no knife edge
GEOMETRIES = sorted(R.GEOMETRIES)


def _folded(case):
    return R.folded_stem(case["stem"]), [B.folded_block(b) for b in case["blocks"]]


@pytest.fixture(scope="module")
def cases():
    """Per geometry: the inputs, the float32 run that picks the masks, the float64 reference under them and its e32 table; computed
    once and left unchanged."""
    out = {}
    for name in GEOMETRIES:
        c = R.make_trunk(name)
        stem, blocks = _folded(c)
        args = (c["im"], stem, blocks, c["counts"], torch.cat(c["g"][:2]), torch.cat(c["g"][2:]))
        r32 = R.trunk(*args, dtype=torch.float32)
        r64 = R.trunk(*args, masks=r32["masks"])
        out[name] = dict(case=c, args=args, r32=r32, r64=r64, e32=R.e32_table(*args, r64))
    yield out
    out.clear()


def test_geometries_are_the_documented_ones(cases):
    want = {"75x107": ((38, 54), (19, 27), (10, 14), (5, 7)), "64x96": ((32, 48), (16, 24), (8, 12), (4, 6))}
    for name, (stem, pool, l2, l3) in want.items():
        nb, H, W = R.GEOMETRIES[name]
        r = cases[name]["r64"]
        assert nb == 4 and R.stem_hw((H, W)) == stem and R.pool_hw(stem) == pool
        assert tuple(r["x0"].shape) == (4, 64) + pool and tuple(r["pre"][0][2].shape) == (4, 256) + pool
        assert tuple(r["feat1"].shape) == (4, 512) + l2 and tuple(r["feat"].shape) == (4, 1024) + l3
    assert (2 * (16 - 1) + 3 > 32) and (2 * (19 - 1) + 3 > 38)           # the last pool window is partial at both
    specs = R.block_specs()
    assert [s[0] for s in specs] == ["layer1.0", "layer1.1", "layer1.2", "layer2.0", "layer2.1", "layer3.0", "layer3.1"]
    assert sum(3 + s[4] for s in specs) == 24                           # 7 x 3 filters and the three projections


def _plain(im, stem, blocks, counts, g_feat, g_feat1):
    """The ordinary network, written without the reference: F.relu and F.max_pool2d decide."""
    v = lambda t: t.double().view(1, -1, 1, 1)
    h = F.max_pool2d(F.relu(F.conv2d(im.double(), stem["w"].double(), None, 2, 3) * v(stem["s"]) + v(stem["b"])), 3, 2, 0, ceil_mode=True)
    ws, feat1 = [], None
    for i, b in enumerate(blocks):
        d = {k: (t.double() if torch.is_tensor(t) else t) for k, t in b.items()}
        ws += [d[n].requires_grad_(True) for n in B.NAMES if d[n] is not None]
        a1 = F.relu(F.conv2d(h, d["w1"], None, d["stride"]) * v(d["s1"]) + v(d["b1"]))
        a2 = F.relu(F.conv2d(a1, d["w2"], None, 1, 1) * v(d["s2"]) + v(d["b2"]))
        skip = h if d["wd"] is None else F.conv2d(h, d["wd"], None, d["stride"]) * v(d["sd"]) + v(d["bd"])
        h = F.relu(F.conv2d(a2, d["w3"]) * v(d["s3"]) + v(d["b3"]) + skip)
        if i == counts[0] + counts[1] - 1:
            feat1 = h
    grads = torch.autograd.grad((h * g_feat.double()).sum() + (feat1 * g_feat1.double()).sum(), ws)
    return h.detach(), feat1.detach(), grads


@pytest.mark.parametrize("name", GEOMETRIES)
def test_own_masks_give_the_ordinary_network(cases, name):
    """``masks=None``: the composition itself -- the stem, the order of the blocks, the tap -- equals plain autograd."""
    args = cases[name]["args"]
    got = R.trunk(*args)
    feat, feat1, grads = _plain(*args)
    assert got["feat"].dtype == torch.float64
    assert B.rel_max(got["feat"], feat) <= 1e-12 and B.rel_max(got["feat1"], feat1) <= 1e-12
    mine = R.tensors(got)
    names = [n for n in mine if n not in ("feat", "feat1")]
    assert len(names) == len(grads) == 24
    for n, g in zip(names, grads):              # block by block in NAMES order: _plain's order
        assert mine[n].shape == g.shape and B.rel_max(mine[n], g) <= 1e-12, n
    for pre, masks in zip(got["pre"], got["masks"]):
        assert all(torch.equal(m, p > 0) for m, p in zip(masks, pre))


@pytest.mark.parametrize("name", GEOMETRIES)
def test_float32_under_shared_masks_sits_at_rounding(cases, name):
    """e32 per tensor, recorded: what max(1e-4, 16 e32) of the GPU test is made of (observed: at most 2e-6, so the block test's
    1e-4 stays the bound in force for every tensor of both geometries)."""
    for n, e in cases[name]["e32"].items():
        record_margin("test_trunk_float32_under_shared_masks[%s]" % name, n, e, SHARED_MASK_BOUND)
        print("%-8s %-14s e32 %.2e   bound in force %.2e" % (name, n, e, R.bound(e)))
        assert e <= SHARED_MASK_BOUND, (name, n, e)


@pytest.mark.parametrize("plant", R.PLANTS)
@pytest.mark.parametrize("name", GEOMETRIES)
def test_every_planted_error_moves_a_tensor_by_ten_bounds(cases, name, plant):
    """A condition, not a measurement: the planted error leaves the forward values bit-equal and moves at least one gradient by
    >= 10 x the bound in force for THAT tensor."""
    c = cases[name]
    broken = R.trunk(*c["args"], masks=c["r32"]["masks"], plant=plant)
    assert torch.equal(broken["feat"], c["r64"]["feat"]) and torch.equal(broken["feat1"], c["r64"]["feat1"])
    for a, b in zip(broken["pre"], c["r64"]["pre"]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    wrong, want = R.tensors(broken), R.tensors(c["r64"])
    ratio = {n: B.rel_max(wrong[n], want[n]) / R.bound(c["e32"][n]) for n in want}
    worst = max(ratio, key=ratio.get)
    record_margin("test_trunk_planted_error[%s-%s]" % (name, plant), "%s, in bounds in force (at least)" % worst, ratio[worst], 10)
    print("%-30s %-8s %-14s %.3g bounds" % (plant, name, worst, ratio[worst]))
    assert ratio[worst] >= 10, (plant, name, ratio)


def test_plants_are_the_documented_ones(cases):
    assert set(R.PLANTS) == {"tap_term_dropped", "tap_premasked", "l3_in_relu_missing_mask", "l1_l2_handover_mask_dropped",
                             "middle_block_handover_dropped", "halves_swapped", "l1_0_wd_from_masked_g"}
    c = cases[GEOMETRIES[0]]
    with pytest.raises(ValueError):
        R.trunk(*c["args"], plant="no_such_error")
    # a plant touches what it names and nothing upstream of it: the projection plant moves layer1.0.wd alone
    wrong = R.tensors(R.trunk(*c["args"], masks=c["r32"]["masks"], plant="l1_0_wd_from_masked_g"))
    moved = [n for n, t in R.tensors(c["r64"]).items() if B.rel_max(wrong[n], t) > 1e-12]
    assert moved == ["layer1.0.wd"], moved


# ---------------------------------------------------------------------------------------------------------------------
# the stem's max pool: what tests/test_gpu_trunk.py compares ops.maxpool3x3s2 with
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tied", [True, False], ids=["tied", "random"])
@pytest.mark.parametrize("hw", R.POOL_HW, ids=lambda hw: "%dx%d" % hw)
def test_max_pool_indices_and_backward_vs_plain_loops(hw, tied):
    x = R.pool_input(hw, tied).double().requires_grad_(True)
    y, idx = F.max_pool2d(x, 3, 2, 0, ceil_mode=True, return_indices=True)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (gx,) = torch.autograd.grad((y * gy).sum(), x)
    ny, nidx, ngx = R.pool_naive(x.detach().numpy(), gy.numpy())
    assert tuple(y.shape[2:]) == R.pool_hw(hw)
    assert np.array_equal(y.detach().numpy(), ny) and np.array_equal(idx.numpy(), nidx)          # ties go to the first in window order
    assert np.abs(gx.numpy() - ngx).max() <= 1e-14 * np.abs(ngx).max()
    if tied:
        xs = x.detach()
        assert bool((xs * 4 == torch.round(xs * 4)).all()) and R.tied_windows(xs) > 0
        if hw != (3, 3):                                                     # (one window per plane: nothing overlaps)
            assert R.tied_windows(xs) > 0.5 and R.shared_winners(nidx) > 0
