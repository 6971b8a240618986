"""The proposal-recall kernel (csrc/proposal_eval.hip) against the host form bit for bit, its status word on malformed tables,
and the proposals the detector test loop keeps (``DetectStep(keep_proposals=True)``, ``proposals_instance_styled.py``)."""
import copy
import pickle

import numpy as np
import pytest
import torch

import proposal_eval_cases as pc
from i2vsgg_amd import proposal_eval as pe

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LIMITS = (1, 64, 65, 300, None)
CAND_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 2000)
GT_COUNTS = (0, 1, 63, 64, 65, 300)
_CACHE = {}


def _grid():
    """Every candidate count against every ground-truth count, one image each (k < m among them); packed and covered on the
    host once for the tests that share it."""
    if "grid" not in _CACHE:
        counts = [(n, m) for n in CAND_COUNTS for m in GT_COUNTS]
        cands, roidb = pc.random_batch(21, counts, size=1200)
        pk = pe.pack(cands, roidb, LIMITS, pc.ALL_AREAS)
        _CACHE["grid"] = (pk, pe.cover_arrays_host(pk))
    return _CACHE["grid"]


def _device(pk, **kw):
    from i2vsgg_amd import ops
    got = ops.proposal_cover(pk.cand_off, pk.cand_box, pk.gt_off, pk.gt_box, pk.gt_area, pk.limits, pk.ranges, device=DEV, **kw)
    assert [t.dtype for t in got] == [torch.float64, torch.int32, torch.int32]
    return tuple(t.cpu().numpy() for t in got)


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("ov", "cand", "step")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        assert np.array_equal(g.view(np.int64) if name == "ov" else g, w.view(np.int64) if name == "ov" else w), (what, name)


def test_device_equals_host_on_every_count():
    pk, want = _grid()
    assert len(pk.cand_off) - 1 == 54 and np.diff(pk.gt_off).max() == 300 and np.diff(pk.cand_off).max() == 2000
    assert (np.diff(pk.cand_off) < np.diff(pk.gt_off)).any()                     # k < m occurs, below every limit
    ov = want[0]
    for a in range(8):
        assert (ov[4, a] >= 0).any(), pc.ALL_AREAS[a]
    assert (ov[4, 0] > 0.9).any() and (want[1][0, 0] == -1).any() and (want[2] > 64).any()
    _same(_device(pk), want, "grid")


def test_two_runs_give_the_same_bits():
    pk, want = _grid()
    _same(_device(pk), _device(pk), "rerun")


@pytest.mark.parametrize("case", ["same_box", "no_overlap", "one_image", "300_images"])
def test_device_equals_host_on_special_batches(case):
    if case == "same_box":                   # every candidate is the same box: every tie goes to the lowest positions
        cands, roidb = pc.random_batch(3, [(300, 65), (65, 64), (64, 5)], size=1200)
        cands = [np.tile(np.float64([[100, 100, 400, 500]]), (len(c), 1)) for c in cands]
    elif case == "no_overlap":               # no candidate overlaps any ground truth: all zeros, lowest free candidate each step
        cands, roidb = pc.random_batch(4, [(257, 64), (64, 65), (5, 9)], size=1200, near=0.0)
        cands = [c + 5000.0 for c in cands]
    elif case == "one_image":
        cands, roidb = pc.random_batch(6, [(257, 17)], size=1200)
    else:
        rng = np.random.default_rng(8)
        cands, roidb = pc.random_batch(7, [(int(n), int(m)) for n, m in zip(rng.integers(0, 81, 300), rng.integers(0, 13, 300))], size=1200)
    pk = pe.pack(cands, roidb, LIMITS, pc.ALL_AREAS)
    want = pe.cover_arrays_host(pk)
    if case == "no_overlap":
        assert (want[0][want[2] >= 0] == 0.0).all() and (want[1] >= 0).any()
    if case == "same_box":
        g0, g1 = pk.gt_off[0], pk.gt_off[1]
        assert np.array_equal(want[1][4, 0, g0:g1], want[2][4, 0, g0:g1])     # step t retires candidate t
    _same(_device(pk), want, case)
    # evaluate() on the device is the same host code behind the cover
    a, b = pe.evaluate(cands, roidb, LIMITS, pc.ALL_AREAS, device=DEV), pe.evaluate(cands, roidb, LIMITS, pc.ALL_AREAS)
    assert set(a) == set(b)
    for key in b:
        if key != "per_class":
            assert np.array_equal(a[key]["recalls"], b[key]["recalls"], equal_nan=True) and np.array_equal(a[key]["gt_overlaps"], b[key]["gt_overlaps"])
    assert all(np.array_equal(a["per_class"][k]["hits"], b["per_class"][k]["hits"]) for k in b["per_class"])


def test_malformed_tables_raise_and_leave_the_other_images_alone():
    """Status-word checks of well-formed launches: a bad image is named and skipped, the others come out as before."""
    from i2vsgg_amd import ops
    from i2vsgg_amd._lib import I2VError
    cands, roidb = pc.random_batch(9, [(40, 6), (70, 9), (0, 4), (65, 12), (30, 3)], size=1200)
    pk = pe.pack(cands, roidb, (5, None), ("all", "small", "large"))
    want = pe.cover_arrays_host(pk)
    G = len(pk.gt_area)

    def run(expect_image, untouched, **tables):
        t = dict(cand_off=pk.cand_off, cand_box=pk.cand_box, gt_off=pk.gt_off)
        t.update(tables)
        out = (torch.full((2, 3, G), -7.0, device=DEV, dtype=torch.float64), torch.full((2, 3, G), -7, device=DEV, dtype=torch.int32),
               torch.full((2, 3, G), -7, device=DEV, dtype=torch.int32))
        with pytest.raises(I2VError, match=r"proposal_cover: .* image %d$" % expect_image):
            ops.proposal_cover(t["cand_off"], t["cand_box"], t["gt_off"], pk.gt_box, pk.gt_area, pk.limits, pk.ranges, device=DEV, out=out)
        got = [x.cpu().numpy() for x in out]
        for i in untouched:
            g0, g1 = pk.gt_off[i], pk.gt_off[i + 1]
            _same([x[:, :, g0:g1] for x in got], [x[:, :, g0:g1] for x in want], "image %d" % i)
        g0, g1 = pk.gt_off[expect_image], min(pk.gt_off[expect_image + 1], G)
        assert all((x[:, :, g0:g1] == -7).all() for x in got)                    # nothing was written for the bad image

    # a decreasing cand_off: image 1 ends before it begins (image 2 then begins elsewhere; 0, 3, 4 are as they were)
    off = pk.cand_off.copy()
    off[2] = off[1] - 1
    run(1, (0, 3, 4), cand_off=off)
    # a gt_off past the end: the last image
    off = pk.gt_off.copy()
    off[-1] = G + 3
    run(4, (0, 1, 2, 3), gt_off=off)
    # an image over the candidate cap (65536 rows of zeros in image 2's place)
    n2 = pe.MAX_CAND + 1
    c0 = int(pk.cand_off[2])
    box = np.concatenate([pk.cand_box[:c0], np.zeros((n2, 4)), pk.cand_box[c0:]])
    off = pk.cand_off.astype(np.int64)
    off[3:] += n2
    run(2, (0, 1, 3, 4), cand_off=off.astype(np.int32), cand_box=box)
    # the well-formed tables still run
    _same(_device(pk), want, "after")


def test_proposal_cover_refuses_the_cpu_and_takes_an_empty_batch():
    from i2vsgg_amd import ops, table_ops
    from i2vsgg_amd._lib import I2VError
    assert ops.proposal_cover is table_ops.proposal_cover
    pk, _ = _grid()
    with pytest.raises(I2VError) as e:
        ops.proposal_cover(pk.cand_off, pk.cand_box, pk.gt_off, pk.gt_box, pk.gt_area, pk.limits, pk.ranges, device="cpu")
    assert "run on the GPU only" in str(e.value) and "proposal_eval.cover_arrays_host is the host form" in str(e.value)
    i32, f64 = lambda *v: np.asarray(v, np.int32), lambda *s: np.zeros(s, np.float64)
    got = ops.proposal_cover(i32(0), f64(0, 4), i32(0), f64(0, 4), f64(0), i32(10), np.float64([[0, 1e10]]), device=DEV)
    assert [tuple(t.shape) for t in got] == [(1, 1, 0)] * 3


@pytest.fixture
def cfg_restored():
    """The global cfg singleton is put back afterwards (the test scripts load a yml into it)."""
    from i2vsgg_amd.model.utils import config as c
    saved = copy.deepcopy(dict(c.cfg))
    yield c
    c._merge_a_into_b(c.AttrDict(saved), c.cfg)


def test_detect_step_keeps_the_proposals_of_detect_frame(cfg_restored):
    """The loop of test_test_scripts_equal_their_frame_by_frame_form: res101, synthetic_10_v at a 192-px shorter side, 64
    proposals, three frames per replay."""
    c = cfg_restored
    from i2vsgg_amd import eval as ev, train
    from i2vsgg_amd._lib import TUNE, lib
    from i2vsgg_amd.roi_data_layer.roibatchLoader import roibatchLoader
    from i2vsgg_amd.roi_data_layer.roidb import combined_roidb
    c.cfg_from_file(c.default_cfg_file("res101"))
    c.cfg_from_list(["ANCHOR_SCALES", "[8, 16, 32]", "ANCHOR_RATIOS", "[0.5,1,2]", "MAX_NUM_GT_BOXES", "30", "TEST.SCALES", "(192,)",
                     "TRAIN.SCALES", "(192,)", "TEST.RPN_POST_NMS_TOP_N", "64"])
    c.cfg.TRAIN.USE_FLIPPED = False
    imdb, roidb, ratio_list, ratio_index = combined_roidb("synthetic_10_v", False)
    net = train.build_instance_styled_net(101, n_cls=imdb.num_classes, device=torch.device(DEV))
    net.eval()
    data = roibatchLoader(roidb, ratio_list, ratio_index, 1, imdb.num_classes, training=False, normalize=False)
    items = [data[i] for i in range(8)]
    groups = {}
    for it in items:
        groups.setdefault(tuple(it[0].shape[-2:]), []).append(it)
    batches = [(torch.stack([it[0].reshape(it[0].shape[-3:]) for it in g]), torch.stack([it[1].reshape(3) for it in g]))
               for g in groups.values()]
    assert len(batches) >= 2 and max(len(b[0]) for b in batches) <= 3
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    try:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)           # no split-K atomics: two forwards of a frame are bit-equal
        z, nb = torch.zeros(1, 1, 5, device=DEV), torch.zeros(1, device=DEV)
        single = [[ev.detect_frame(net, im[f:f + 1].to(DEV), info[f:f + 1].to(DEV), z, nb, keep_proposals=True) for f in range(len(im))]
                  for im, info in batches]
        plain_single = ev.detect_frame(net, batches[0][0][:1].to(DEV), batches[0][1][:1].to(DEV), z, nb)
        keeping = ev.DetectStep(net, frames=3, device=DEV, keep_proposals=True)
        plain = ev.DetectStep(net, frames=3, device=DEV)
        assert plain.props is None and plain._props_host is None and keeping.props.shape == (3, 64, 5)
        kept = [keeping(im, info) for im, info in batches]
        today = [plain(im, info) for im, info in batches]
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)
    assert isinstance(plain_single, list) and len(plain_single) == imdb.num_classes           # without the keyword: today's value
    n_props = 0
    for b, (im, info) in enumerate(batches):
        assert isinstance(today[b], list) and len(today[b]) == len(im) and len(today[b][0]) == imdb.num_classes
        res, props = kept[b]
        assert len(res) == len(props) == len(im)
        for f in range(len(im)):
            want_res, want_props = single[b][f]
            assert props[f].dtype == np.float32 and props[f].ndim == 2 and props[f].shape[1] == 4 and 0 < len(props[f]) <= 64
            assert np.array_equal(props[f], want_props), (b, f)
            assert (props[f][-1] != 0).any()                                                    # the padding is gone
            for j in range(imdb.num_classes):
                assert np.array_equal(res[f][j], today[b][f][j]) and np.array_equal(res[f][j], want_res[j]), (b, f, j)
            n_props += len(props[f])
    assert n_props > 0
    # the padding rows: trailing all-zero boxes only
    rois = np.float32([[0, 1, 2, 3, 4], [0, 0, 0, 0, 0], [0, 5, 6, 7, 8], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
    assert ev.trim_proposals(rois).tolist() == [[1, 2, 3, 4], [0, 0, 0, 0], [5, 6, 7, 8]] and ev.trim_proposals(rois[3:]).shape == (0, 4)


def test_test_script_saves_and_scores_its_proposals(cfg_restored, tmp_path, capsys):
    """proposals_instance_styled.py, the detection test loop with the proposals kept, on a small synthetic roidb whose frames differ
    in size (groups of two leave out of loader order, short groups at the end)."""
    import proposals_instance_styled as ps
    import test_instance_styled as td
    from i2vsgg_amd._lib import TUNE, lib
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    args = ["--net", "res50", "--imdbval_name", "synthetic_7_v", "--scale", "192", "--frames", "2", "--output_dir", str(tmp_path),
            "--set", "TEST.RPN_POST_NMS_TOP_N", "64"]
    other = lambda frames, d: args[:7] + [frames] + args[8:9] + [str(tmp_path / d)] + args[10:]
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    try:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)           # no split-K atomics: two forwards of a frame are bit-equal
        got_boxes, got_props, got_res = ps.main(args)
        out = capsys.readouterr().out
        _, one_props, _ = ps.main(other("1", "one"))             # frame by frame
        plain_boxes = td.main(other("2", "plain"))               # the detection test loop itself
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)
    with open(tmp_path / "res50" / "synthetic" / "proposals.pkl", "rb") as f:
        props = pickle.load(f)
    imdb = get_imdb("synthetic_7_v")
    assert len(props) == 7 and all(p.dtype == np.float64 and p.ndim == 2 and p.shape[1] == 4 and 0 < len(p) <= 64 for p in props)
    for p, (h, w) in zip(props, imdb._sizes):                     # image coordinates: inside the native frame (clipped at the scaled one)
        assert p.min() >= 0 and p[:, 2].max() <= w + 1 and p[:, 3].max() <= h + 1
    host = pe.evaluate(props, imdb.roidb, num_classes=imdb.num_classes)
    dev = pe.evaluate(props, imdb.roidb, num_classes=imdb.num_classes, device=DEV)
    lines = [x for x in out.splitlines() if x.startswith("AR@")]
    assert len(lines) == 20 and ("wrote %s" % (tmp_path / "res50" / "synthetic" / "proposals.pkl")) in out
    for key, line in zip([k for k in host if k != "per_class"], lines):
        assert np.array_equal(dev[key]["recalls"], host[key]["recalls"], equal_nan=True) and dev[key]["num_pos"] == host[key]["num_pos"]
        assert np.array_equal(dev[key]["gt_overlaps"], host[key]["gt_overlaps"])
        assert line.startswith("AR@%-5s %-8s = %.4f" % ("all" if key[0] is None else key[0], key[1], host[key]["ar"])), (key, line)
    line, = [x for x in lines if x.startswith("AR@all") and " all " in x]
    r50 = float(line.split("recall@0.50 = ")[1].split()[0])
    assert 0.0 <= r50 <= 1.0 and abs(r50 - host[(None, "all")]["recalls"][0]) < 1e-4
    # what it returns is what it wrote and printed; the frame-by-frame form keeps the same proposals, image by image
    assert len(got_props) == 7 and all(np.array_equal(a, b) for a, b in zip(got_props, props))
    assert all(np.array_equal(got_res[k]["recalls"], host[k]["recalls"], equal_nan=True) for k in host if k != "per_class")
    assert len(one_props) == 7 and all(np.array_equal(a, b) for a, b in zip(one_props, props))
    # one pass gives both files: its detections.pkl is the detection test loop's, which writes no proposals.pkl
    with open(tmp_path / "res50" / "synthetic" / "detections.pkl", "rb") as f:
        saved = pickle.load(f)
    n_det = 0
    for j in range(1, imdb.num_classes):
        for i in range(7):
            assert np.array_equal(saved[j][i], plain_boxes[j][i]) and np.array_equal(got_boxes[j][i], plain_boxes[j][i]), (j, i)
            n_det += len(saved[j][i])
    assert n_det > 0 and (tmp_path / "plain" / "res50" / "synthetic" / "detections.pkl").exists()
    assert not (tmp_path / "plain" / "res50" / "synthetic" / "proposals.pkl").exists()


def test_an_image_of_thousands_of_ground_truths_takes_the_large_lds_path():
    """4000 ground truths in one image: 56 KB of LDS per cell, above the 48 KB below which no limit has to be raised; fewer
    candidates than ground truths in it, and a small image beside it in the same launch."""
    cands, roidb = pc.random_batch(12, [(600, 4000), (70, 9)], size=1200)
    pk = pe.pack(cands, roidb, (65, None), ("all", "large"))
    assert np.diff(pk.gt_off).max() == 4000 and 14 * 4000 > 48 * 1024
    want = pe.cover_arrays_host(pk)
    assert (want[1] == -1).any() and want[2].max() == 3999
    _same(_device(pk), want, "large lds")


def test_proposal_cover_refuses_a_limit_below_one():
    from i2vsgg_amd import ops
    pk, _ = _grid()
    for bad in ((0,), (5, -1)):
        with pytest.raises(ValueError, match="every limit is >= 1"):
            ops.proposal_cover(pk.cand_off, pk.cand_box, pk.gt_off, pk.gt_box, pk.gt_area, np.asarray(bad, np.int32), pk.ranges, device=DEV)
