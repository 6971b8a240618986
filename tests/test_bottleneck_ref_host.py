"""The masked float64 reference of the bottleneck chain (tests/bottleneck_ref.py) checked on its own, on the CPU: against a plainly
written F.relu / F.conv2d network, against float32 torch under shared masks (no knife edge left), and against every planted
error -- each must move a gradient by 10x the bound tests/test_gpu_bottleneck_bwd.py asserts, which is what gives that test teeth."""
import pytest
import torch
import torch.nn.functional as F

import bottleneck_ref as R
from conftest import record_margin

# what tests/test_gpu_bottleneck_bwd.py holds every gradient tensor to (WINOGRAD_REL where the path crosses a Winograd kernel,
# the direct pieces' 1e-4 elsewhere: the same number)
GPU_BOUND = 1e-4
SHARED_MASK_BOUND = 1e-5        # float32 torch against the masked reference
CASES = sorted(R.CASES)


@pytest.fixture(scope="module")
def cases():
    """Per case: the inputs, the folded blocks, the float32 run that picks the masks and the masked float64 reference; computed
    once and left unchanged."""
    out = {}
    for name in CASES:
        c = R.make_case(name)
        blocks = [R.folded_block(b) for b in c["blocks"]]
        in_mask = (c["x"] > 0) if c["in_relu"] else None
        r32 = R.chain(c["x"], blocks, c["gout"], in_mask=in_mask, dtype=torch.float32)
        r64 = R.chain(c["x"], blocks, c["gout"], masks=r32["masks"], in_mask=in_mask)
        out[name] = dict(case=c, blocks=blocks, in_mask=in_mask, r32=r32, r64=r64)
    yield out
    out.clear()


def _plain(x, blocks, gout, in_relu):
    """The ordinary network, written without the module: F.relu decides."""
    leaf = x.double().requires_grad_(True)
    h = F.relu(leaf) if in_relu else leaf           # x is a ReLU output already: relu(x) == x, and its gradient carries x > 0
    ws = []
    for b in blocks:
        d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in b.items()}
        for n in R.NAMES:
            if d[n] is not None:
                ws.append(d[n].requires_grad_(True))
        v = lambda t: t.view(1, -1, 1, 1)
        a1 = F.relu(F.conv2d(h, d["w1"], None, d["stride"]) * v(d["s1"]) + v(d["b1"]))
        a2 = F.relu(F.conv2d(a1, d["w2"], None, 1, 1) * v(d["s2"]) + v(d["b2"]))
        skip = h if d["wd"] is None else F.conv2d(h, d["wd"], None, d["stride"]) * v(d["sd"]) + v(d["bd"])
        h = F.relu(F.conv2d(a2, d["w3"]) * v(d["s3"]) + v(d["b3"]) + skip)
    grads = torch.autograd.grad((h * gout.double()).sum(), [leaf] + ws)
    return h.detach(), grads


@pytest.mark.parametrize("name", CASES)
def test_own_masks_give_the_ordinary_network(cases, name):
    c = cases[name]
    got = R.chain(c["case"]["x"], c["blocks"], c["case"]["gout"], in_mask=c["in_mask"])
    out, grads = _plain(c["case"]["x"], c["blocks"], c["case"]["gout"], c["case"]["in_relu"])
    assert got["out"].dtype == torch.float64 and R.rel_max(got["out"], out) <= 1e-12
    mine = R.gradients(got)
    assert len(mine) == len(grads) and len(mine) == 1 + sum(3 + (b["wd"] is not None) for b in c["blocks"])
    for (n, a), b in zip(mine.items(), grads):          # gx, then the filters block by block in NAMES order: _plain's order
        assert a.shape == b.shape and R.rel_max(a, b) <= 1e-12, n
    for (p1, p2, p3), masks in zip(got["pre"], got["masks"]):
        assert all(torch.equal(m, p > 0) for m, p in zip(masks, (p1, p2, p3)))


@pytest.mark.parametrize("name", CASES)
def test_float32_under_shared_masks_has_no_knife_edge(cases, name):
    """float32 torch picks the masks, the float64 reference computes under them: every gradient within 1e-5 of its largest
    element (observed 1e-6), where the block stack test has to allow 5e-2 for references that pick their own."""
    c = cases[name]
    want = R.gradients(c["r64"])
    for n, got in R.gradients(c["r32"]).items():
        err = R.rel_max(got, want[n])
        record_margin("test_float32_under_shared_masks[%s]" % name, n, err, SHARED_MASK_BOUND)
        print("%-18s %-8s %.2e" % (name, n, err))
        assert err <= SHARED_MASK_BOUND, (name, n, err)
    assert R.rel_max(c["r32"]["out"], c["r64"]["out"]) <= SHARED_MASK_BOUND


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_planted_error_moves_a_gradient_by_ten_bounds(cases, mutation):
    """A condition, not a measurement: on every case where the term exists, the planted error moves at least one gradient tensor
    by >= 10 x the bound the GPU test asserts for it."""
    seen = 0
    for name in CASES:
        if not R.mutation_applies(mutation, name):
            continue
        c = cases[name]
        broken = R.chain(c["case"]["x"], c["blocks"], c["case"]["gout"], masks=c["r32"]["masks"], in_mask=c["in_mask"], mutate=mutation)
        assert R.rel_max(broken["out"], c["r64"]["out"]) <= 1e-12       # the forward is the unbroken one: only the backward errs
        wrong, want = R.gradients(broken), R.gradients(c["r64"])
        moved = {n: R.rel_max(wrong[n], want[n]) for n in want}
        worst = max(moved, key=moved.get)
        record_margin("test_every_planted_error[%s]" % mutation, "%s %s (at least)" % (name, worst), moved[worst], 10 * GPU_BOUND)
        print("%-24s %-18s %-8s %.2e   (>= %.0e)" % (mutation, name, worst, moved[worst], 10 * GPU_BOUND))
        assert moved[worst] >= 10 * GPU_BOUND, (mutation, name, moved)
        seen += 1
    assert seen >= (1 if mutation == "handover_mask_dropped" else 3)


def test_mutations_and_cases_are_the_documented_ones():
    assert set(R.MUTATIONS) == {"s3_1pct", "s1_one_channel_5pct", "m1_last_column_on", "mo_not_applied_to_skip", "proj_scale_dropped",
                                "handover_mask_dropped", "wgrad_row_scale_dropped"}
    assert [n for n in CASES if R.mutation_applies("proj_scale_dropped", n)] == ["hand_over", "projection", "strided"]
    assert [n for n in CASES if R.mutation_applies("handover_mask_dropped", n)] == ["hand_over"]
    with pytest.raises(ValueError):
        c = R.make_case("tiny_map")
        R.chain(c["x"], [R.folded_block(b) for b in c["blocks"]], c["gout"], mutate="no_such_error")
