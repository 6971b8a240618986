"""Video relation NMS on the MI355X: csrc/video_nms.hip (ops.video_relation_nms) against the host form of
i2vsgg_amd.video.suppress.  keep and by are equal, vol and by_ov equal in every bit: both forms add the same float64 terms in
the same order, one accumulator per sum, so there is no tolerance anywhere."""
import copy
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import golden  # noqa: E402
import video_nms_cases as nc  # noqa: E402

DEV = "cuda:0"
CASES = dict((c.name, c) for c in nc.built_cases())
RUNS = [(n, None) for n in CASES] + [("sizes", 1.0), ("sizes", 0.0), ("frames", 0.9), ("big", 0.95)]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _device(pk, T, **kw):
    from i2vsgg_amd import ops
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return [t.cpu().numpy() for t in ops.video_relation_nms(pk.cell_off, pk.rel, pk.boxes, T, device=DEV, **kw)]


def _same(got, want):
    keep, by, by_ov, vol = got
    assert keep.dtype == np.int32 and by.dtype == np.int32 and vol.shape == want[3].shape
    assert (keep == want[0]).all() and (by == want[1]).all()
    assert (_bits(by_ov) == _bits(want[2])).all() and (_bits(vol) == _bits(want[3])).all()


@pytest.fixture(scope="module")
def host():
    """Every case packed once and the host form's answer per (case, T); nobody writes to either."""
    from i2vsgg_amd import video
    pks = dict((n, video.pack_nms(c.prediction, c.pool)) for n, c in CASES.items())
    return pks, dict(((n, T), video.suppress_arrays_host(pks[n], CASES[n].T if T is None else T)) for n, T in RUNS)


@pytest.mark.parametrize("name,T", RUNS)
def test_device_equals_the_host_form(host, name, T):
    pks, want = host
    got = _device(pks[name], CASES[name].T if T is None else T)
    _same(got, want[name, T])
    if name == "big":
        assert len(pks[name].rel) == 1025 and 1 < got[0].sum() < 1025
    if (name, T) == ("sizes", 1.0):
        assert got[0].all()                              # nothing exceeds 1: every row is compared with every later one
    if (name, T) == ("sizes", None):
        assert set(np.diff(pks[name].cell_off).tolist()) == set(nc.CELL_SIZES)
    if name.startswith("edge"):                          # cells of exactly the workgroup's 256 lanes, and one row fewer
        assert sorted(np.diff(pks[name].cell_off).tolist()) == [256 if name == "edge_wide" else 255, 256] and 2 < got[0].sum() < 500


def test_two_runs_give_the_same_bits(host):
    pks, _ = host
    for name in ("big", "fractional", "multi"):
        a, b = _device(pks[name], CASES[name].T), _device(pks[name], CASES[name].T)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_golden_decisions_on_the_device():
    from i2vsgg_amd import video
    g = golden("video_nms")
    n = int(g["n_cases"])
    for k in range(n):
        pk = video.PackedNMS([], None, g["c%d_cell_off" % k], g["c%d_rel" % k], g["c%d_score" % k], g["c%d_boxes" % k], None, None, None)
        keep, by, by_ov, _ = _device(pk, float(g["c%d_T" % k]))
        assert (keep == g["c%d_keep" % k]).all() and (by == g["c%d_by" % k]).all(), k
        ref = g["c%d_by_ov" % k]
        if k < n - 2:
            assert (_bits(by_ov) == _bits(ref)).all(), k
        else:
            hit = by >= 0
            assert (by_ov[~hit] == -1.0).all() and (np.abs(by_ov[hit] - ref[hit]) <= 1e-12 * ref[hit]).all(), k


def test_malformed_tables_are_reported_and_not_followed(host):
    """A bad offset, a span past ``boxes``, a length that disagrees with the duration: the cell is named, nothing of it is written,
    and the other cells are what they were."""
    from i2vsgg_amd._lib import I2VError
    pks, want = host
    pk, good = pks["multi"], want["multi", None]
    T, C, R, NB = CASES["multi"].T, len(pks["multi"].cell_off) - 1, len(pks["multi"].rel), len(pks["multi"].boxes)
    off = pk.cell_off
    row = lambda c: int(off[c])                          # the first row of a cell

    def check(bad_cells, cell_off=None, rel=None):
        bad = copy.copy(pk)
        bad.cell_off = off if cell_off is None else cell_off
        bad.rel = pk.rel if rel is None else rel
        with pytest.raises(I2VError, match="video_relation_nms: .* cell %d" % max(bad_cells)):
            _device(bad, T)
        keep, by, by_ov, vol = _device(bad, T, read_status=False)
        for c in range(C):
            r0, r1 = int(off[c]), int(off[c + 1])
            if c in bad_cells:
                assert not keep[r0:r1].any() and (by[r0:r1] == -1).all() and (by_ov[r0:r1] == -1.0).all() and (vol[r0:r1] == 0.0).all()
            else:
                _same((keep[r0:r1], by[r0:r1], by_ov[r0:r1], vol[r0:r1]), [x[r0:r1] for x in good])

    def rel_with(r, col, value):
        rel = pk.rel.copy()
        rel[r, col] = value
        return rel
    sizes = np.diff(off).tolist()
    assert C == 5 and sorted(sizes[:3]) == [1, 17, 30] and sizes[3:] == [70, 1]
    a = sizes.index(30)
    past = off.copy()
    past[2] = R + 5                                      # cell 1 ends past the table, cell 2 begins there (and ends before that)
    check({1, 2}, cell_off=past)
    neg = off.copy()
    neg[0] = -1
    check({0}, cell_off=neg)
    check({1}, rel=rel_with(row(1), 6, NB - 1))          # a subject span past ``boxes`` (the cell's trajectories are longer than 1)
    check({3}, rel=rel_with(row(3) + 2, 8, -4))          # a negative object offset
    check({a}, rel=rel_with(row(a) + 5, 7, int(pk.rel[row(a) + 5, 7]) + 1))            # one box more than fend - fstart
    check({a}, rel=rel_with(row(a) + 29, 5, int(pk.rel[row(a) + 29, 5]) - 1))          # a duration one frame shorter than both
    check({4}, rel=rel_with(row(4), 9, 0))               # an empty object trajectory for a duration of one frame
    _same(_device(pk, T), good)                          # and the op runs after it


def test_a_cell_of_4097_given_by_offsets_alone():
    """4097 rows that are one relation 4097 times: as one cell it is reported; as 4096 + 1 it runs, and the first row suppresses
    the other 4095 (ov = 1)."""
    from i2vsgg_amd import video
    from i2vsgg_amd._lib import I2VError
    one = video.pack_nms({"v": [nc.rel((1, 2, 3), 0.5, 0, [[0, 0, 9, 9]] * 3, [[5, 5, 30, 30]] * 3)]})
    pk = copy.copy(one)
    pk.rel = np.repeat(one.rel, 4097, 0)
    pk.cell_off = np.asarray([0, 4097], np.int32)
    with pytest.raises(I2VError, match="video_relation_nms: .*more than 4096 relations.* cell 0"):
        _device(pk, 0.5)
    keep, by, by_ov, vol = _device(pk, 0.5, read_status=False)
    assert not keep.any() and (by == -1).all() and (vol == 0.0).all()
    pk.cell_off = np.asarray([0, 4096, 4097], np.int32)
    keep, by, by_ov, vol = _device(pk, 0.5)
    assert keep.tolist() == [1] + [0] * 4095 + [1] and by.tolist() == [-1] + [0] * 4095 + [-1]
    assert (by_ov[1:4096] == 1.0).all() and (vol == [300.0, 2028.0]).all()
    _same((keep, by, by_ov, vol), video.suppress_arrays_host(pk, 0.5))


def test_binding_checks_and_empty_tables():
    from i2vsgg_amd import ops, video
    from i2vsgg_amd._lib import I2VError
    pk = video.pack_nms(CASES["chain"].prediction)
    with pytest.raises(I2VError, match="GPU only"):
        ops.video_relation_nms(pk.cell_off, pk.rel, pk.boxes, 0.5, device="cpu")
    with pytest.raises(ValueError, match="sizes do not agree"):
        ops.video_relation_nms(pk.cell_off, pk.rel.reshape(-1)[:-1], pk.boxes, 0.5, device=DEV)
    with pytest.raises(I2VError, match="threshold lies in \\[0, 1\\]"):
        ops.video_relation_nms(pk.cell_off, pk.rel, pk.boxes, 1.5, device=DEV)
    empty = video.pack_nms({"v": [], "w": []})
    res = _device(empty, 0.5)
    assert [len(x) for x in res] == [0, 0, 0, 0] and len(empty.cell_off) == 1
    out, info = video.suppress({"v": []}, 0.5, device=DEV)
    assert out == {"v": []} and info["v"]["kept"] == 0


def test_suppress_on_the_device_equals_the_host():
    from i2vsgg_amd import video
    for case in [CASES[n] for n in ("multi", "fractional", "sizes", "pool", "cap", "tie")]:
        a, ia = video.suppress(case.prediction, case.T, case.cap, case.pool, device=DEV)
        b, ib = video.suppress(case.prediction, case.T, case.cap, case.pool, device=None)
        assert ia == ib and list(a) == list(b)
        for vid in a:
            assert len(a[vid]) == len(b[vid]) and all(x is y for x, y in zip(a[vid], b[vid])), (case.name, vid)
    pred, gt = nc.duplicates_case()
    out, info = video.suppress(pred, 0.7, device=DEV)
    assert all(len(out[vid]) == 4 for vid in pred) and video.evaluate(out, gt, device=DEV)[0] == 1.0


def test_script_writes_what_the_cpu_run_writes(tmp_path):
    """video_sgg_emb.py --relations ... --rel_nms 0.7: the association and the suppression on the GPU write the file the --cpu
    run writes; without the flag the file is the one of before."""
    from i2vsgg_amd import synthetic as syn, video
    import video_sgg_emb as tv
    results = nc.frame_results(syn.video_frames(312, 40, integer=True, quant=64))
    pkl = str(tmp_path / "relations.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(results, f)
    out = str(tmp_path / "video_relations.json")
    files = []
    for extra in (["--rel_nms", "0.7"], ["--rel_nms", "0.7", "--cpu"], [], ["--cpu"]):
        tv.main(["--relations", pkl] + extra)
        with open(out, "rb") as f:
            files.append(f.read())
    assert files[0] == files[1] and files[2] == files[3] and files[0] != files[2]
    fr = video.from_frame_results(results, dict((p, ("0", k)) for k, p in enumerate(sorted(results))))
    assert files[2] == json.dumps(video.associate(fr)).encode()
    assert 0 < len(json.loads(files[0].decode())["0"]) < len(json.loads(files[2].decode())["0"])
