"""i2vsgg_amd/launch.py: which arena, split workspace and scratch buffer a launch gets -- nesting of entered contexts, the
launch stream's default context, the ordered-sums switch of a context and the side context of the filter-gradient branch.
Tiny tensors, no network, no step object.  Needs a real MI355X: `pytest -m gpu`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def launch():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from i2vsgg_amd import launch as m
    return m


@pytest.fixture(autouse=True)
def no_residue(launch):
    """The default contexts these tests create (a 48 MB slab each) go with the test: later tests find the process as it was."""
    saved = dict(launch._DEFAULTS)
    yield
    launch._DEFAULTS.clear()
    launch._DEFAULTS.update(saved)
    torch.cuda.synchronize()


def _owned(launch):
    """(arena, split buffer pointer, pointer of the scratch buffer tagged "t") as a wrapper would get them now."""
    return launch.arena(), launch.split_buffer(DEV).data_ptr(), launch.workspace(256, DEV, "t").data_ptr()


def _of(ctx):
    return ctx.arena, ctx.split.buf.data_ptr(), ctx.scratch["t"].data_ptr()


@pytest.mark.parametrize("fail", [False, True])
def test_entered_contexts_nest_and_unwind(launch, fail):
    A, B = launch.LaunchContext(DEV), launch.LaunchContext(DEV)
    with A:
        assert _owned(launch) == _of(A) and A.arena is not None
        try:
            with B:
                assert _owned(launch) == _of(B)
                assert B.arena is not A.arena and _of(B)[1:] != _of(A)[1:]
                if fail:
                    raise KeyError("inside B")
        except KeyError:
            assert fail
        assert launch.current() is A and _owned(launch) == _of(A)
    default = launch.current(DEV)
    assert default is not A and default is not B and default.arena is None
    got = _owned(launch)
    assert got == _of(default) and got[0] is None
    assert got[1] not in (_of(A)[1], _of(B)[1]) and got[2] not in (_of(A)[2], _of(B)[2])
    if fail:        # an exception that leaves both blocks at once
        with pytest.raises(KeyError):
            with A, B:
                raise KeyError("inside B")
        assert launch.current(DEV) is default


def test_default_context_belongs_to_the_launch_stream(launch):
    # streams the step objects use anyway (no new ones: role streams are never destroyed); their default contexts start empty here
    s1, s2, s3 = launch.role_stream(DEV, ("frame", 0)), launch.role_stream(DEV, ("frame", 1)), launch.role_stream(DEV, "side")
    for s in (s1, s2, s3):
        launch._DEFAULTS.pop((DEV.index, s.cuda_stream), None)
    with torch.cuda.stream(s1):
        c1 = launch.current(DEV)
        w1, b1 = launch.workspace(256, DEV, "t"), launch.split_buffer(DEV)
        assert launch.workspace(256, DEV, "t") is w1 and launch.split_buffer(DEV) is b1
        assert launch.current(DEV) is c1 and c1.arena is None and launch.arena() is None
    with torch.cuda.stream(s2):
        w2, b2 = launch.workspace(256, DEV, "t"), launch.split_buffer(DEV)
        assert launch.current(DEV) is not c1
    assert w1.data_ptr() != w2.data_ptr() and b1.data_ptr() != b2.data_ptr()
    with torch.cuda.stream(s1):       # back on the first stream: its buffers again; grow-only
        assert launch.workspace(256, DEV, "t") is w1 and launch.split_buffer(DEV) is b1
        big = launch.workspace(1 << 16, DEV, "t")
        assert big.numel() >= 1 << 16 and big is not w1
        assert launch.workspace(512, DEV, "t") is big
    with torch.cuda.stream(s3):       # scratch alone allocates no split slab
        launch.workspace(256, DEV, "t")
        assert launch.current(DEV).split is None and "t" in launch.current(DEV).scratch


def test_ordered_context_switches_split_atomics_only_from_the_process_default(launch, monkeypatch):
    from i2vsgg_amd._lib import TUNE, lib
    key = TUNE["I2V_SPLIT_ATOMICS"]
    monkeypatch.setattr(launch, "ORDERED_SUMS", True)
    old = lib.i2v_get_tuning(key)
    ctx = launch.LaunchContext(DEV, arena=False, ordered=True)
    try:
        assert lib.i2v_set_tuning(key, 2) == 0
        with ctx:
            assert lib.i2v_get_tuning(key) == 0
        assert lib.i2v_get_tuning(key) == 2
        with pytest.raises(KeyError):
            with ctx:
                raise KeyError("restored on the way out too")
        assert lib.i2v_get_tuning(key) == 2
        assert lib.i2v_set_tuning(key, 1) == 0       # an explicit "always atomics" is the user's to keep
        with ctx:
            assert lib.i2v_get_tuning(key) == 1
        assert lib.i2v_get_tuning(key) == 1
        assert lib.i2v_set_tuning(key, 2) == 0
        monkeypatch.setattr(launch, "ORDERED_SUMS", False)      # I2V_ORDERED_SUMS=0: ordered=True is ignored
        with ctx:
            assert lib.i2v_get_tuning(key) == 2
    finally:
        lib.i2v_set_tuning(key, old)      # the process default, 2


def test_side_branch_runs_under_a_child_of_the_forking_context(launch):
    """One 64 -> 64 channel 1x1 filter gradient over 1x16x16 = 256 pixels (above 224 the launcher splits the reduction: zeros
    from the arena, beta = 1, the ordered sum through the split workspace) on the side branch against the same call on the main
    stream under the parent context: the same bits."""
    from i2vsgg_amd import ops
    torch.manual_seed(5)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    x, g = cl(torch.randn(1, 64, 16, 16, device=DEV)), cl(torch.randn(1, 64, 16, 16, device=DEV))
    parent = launch.LaunchContext(DEV, ordered=True)
    parent.arena = launch.ZeroArena(1 << 16, DEV)
    wgrad = lambda: ops._conv_wgrad_raw(x, g, (64, 64, 1, 1), 1, 0)
    with parent, torch.no_grad():
        want = wgrad().clone()
        assert parent.arena.off == 64 * 64               # the zeros came from the arena

    side = launch.SideBranch(launch.role_stream(DEV, "wgrad"))       # the role train.InstanceStyleDStep gives it
    seen = {}

    def on_the_side():
        seen["stream"] = torch.cuda.current_stream().cuda_stream
        seen["ctx"], seen["owned"] = launch.current(), _owned(launch)
        seen["off"] = parent.arena.off
        assert launch.arena().take_flat(64) is not None
        seen["off_after_take"] = parent.arena.off
        return wgrad()

    with parent, torch.no_grad():
        arena, p_split, p_scratch = _owned(launch)
        mine = arena.take_flat(128).fill_(1.0)           # taken before the fork: the child must neither clear nor rewind it
        got = side.run(on_the_side, x, g)
        assert launch.current() is parent and side.kept == [(x, g)]
        with torch.cuda.stream(side.stream), pytest.raises(RuntimeError, match="is the current stream"):
            side.join()
        assert side.kept == [(x, g)]
        side.join()
        assert side.kept == []
        torch.cuda.synchronize()
        assert bool((mine == 1.0).all())
        assert parent.arena.off == 128 + 64 + 64 * 64
    child = seen["ctx"]
    assert child is parent.side() and child is not parent and child.borrows_arena
    assert seen["stream"] == side.stream.cuda_stream != torch.cuda.current_stream().cuda_stream
    assert seen["owned"][0] is arena is parent.arena
    assert (seen["off"], seen["off_after_take"]) == (128, 128 + 64)
    assert seen["owned"][1] != p_split and seen["owned"][2] != p_scratch
    assert seen["owned"][1:] == _of(child)[1:]
    assert got.data_ptr() != want.data_ptr() and torch.equal(got, want)
    assert float(want.abs().max()) > 0
