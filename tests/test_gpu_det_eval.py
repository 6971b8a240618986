"""The detection-evaluation kernels (csrc/det_eval.hip) against the reference's voc_eval (tests/golden/det_eval.npz) and,
on a larger seeded set with heavy score ties and on small ones around the sort's 4096-key tile, against the host form of
i2vsgg_amd.detection_eval bit for bit."""
import copy

import numpy as np
import pytest
import torch

import det_eval_golden as dg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _same_doubles(a, b):
    """The same bits, or a nan on both sides (0 / 0: the sign and payload of the nan are the divider's own)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


@pytest.fixture(scope="module")
def fresh():
    from i2vsgg_amd import detection_eval as de
    all_boxes, roidb, classes = dg.fresh_set()
    return de.pack(all_boxes, roidb, len(classes))


def test_kernels_match_the_reference():
    from i2vsgg_amd import detection_eval as de
    g, all_boxes, roidb, classes = dg.golden_inputs()
    pk = de.pack(all_boxes, roidb, len(classes))
    for t, thr in enumerate(g["thresholds"]):
        flag, ovmax, jmax, cur = de.evaluate_packed(pk, float(thr), device=DEV)
        dg.check_against_reference(g, pk, t, cur)
        hflag, hov, hj = de.match_arrays_host(pk, float(thr))
        assert np.array_equal(flag, hflag) and np.array_equal(jmax, hj) and np.array_equal(_bits(ovmax), _bits(hov))
        if thr == 0.5:
            assert (ovmax == 0.5).any() and (flag[ovmax == 0.5] == de.FP).all() and (jmax > 63).any()
    res = de.evaluate(all_boxes, roidb, classes, 0.5, device=DEV)
    assert np.isnan(res["mean_ap"]) and res["mean_ap_present"] == np.mean(res["aps"][:-1])


def test_kernels_equal_the_host_form_on_a_large_set_with_ties(fresh):
    from i2vsgg_amd import detection_eval as de
    pk = fresh
    n_per, seg_n, seg_g = np.diff(pk.cls_off), np.diff(pk.seg_det_off), np.diff(pk.gt_off)
    assert pk.n_images >= 2000 and pk.n_classes == 15 and n_per.max() > 200000 and (n_per == 0).any()
    assert seg_n.max() == 100 and seg_g.max() >= 65 and seg_g.max() <= 80 and (seg_g[pk.seg_gt] == 0).any()
    assert ((n_per > 0) & (pk.npos == 0)).any()
    keys = pk.det_key[pk.cls_off[0]:pk.cls_off[1]]
    assert len(np.unique(keys)) <= 201                   # heavy ties: 200 000 detections share 201 scores
    assert (pk.det_box * 4 != np.round(pk.det_box * 4)).any()
    flag, ovmax, jmax, cur = de.evaluate_packed(pk, 0.5, device=DEV)
    hflag, hov, hj = de.match_arrays_host(pk, 0.5)
    hcur = de.curve_arrays_host(pk, hflag)
    print("detections %d, segments %d, tp %d, fp %d, ignored %d" % (len(flag), len(seg_n), (hflag == de.TP).sum(),
                                                                     (hflag == de.FP).sum(), (hflag == de.IGNORED).sum()))
    assert (hflag == de.TP).sum() > 1000 and (hflag == de.IGNORED).sum() > 100
    assert np.array_equal(flag, hflag), int((flag != hflag).sum())
    assert np.array_equal(jmax, hj), int((jmax != hj).sum())
    assert np.array_equal(_bits(ovmax), _bits(hov)), int((_bits(ovmax) != _bits(hov)).sum())
    for name in ("perm", "cum_tp", "cum_fp"):
        assert np.array_equal(cur[name], hcur[name]), name
    for name in ("rec", "prec", "ap_area", "ap_11pt"):
        assert _same_doubles(cur[name], hcur[name]), name
    assert np.isnan(cur["ap_area"]).sum() == 1 and (cur["ap_area"][~np.isnan(cur["ap_area"])] > 0).sum() >= 13


@pytest.mark.parametrize("n_cls", [1, 2])
@pytest.mark.parametrize("n_det", [1, 4095, 4096, 4097, 8193])
def test_curve_equals_the_host_form_around_the_sort_tile(n_det, n_cls):
    """det_eval_curve between the golden set and the large one: one key short of a 4096-key sort tile, exactly one, one
    more (two tiles, the first global step) and three tiles' worth (four, one of them all padding), as one class and as
    two classes whose boundary lies inside a tile; at most 7 distinct scores, so the order rests on the positions."""
    from i2vsgg_amd import detection_eval as de, ops
    rng = np.random.RandomState(1000 * n_cls + n_det)
    det_key = rng.choice(np.array([-2000, -1, 0, 1, 499, 500, 999], np.int32), n_det)
    assert len(np.unique(det_key)) <= 7
    cls_off = np.array([0, n_det] if n_cls == 1 else [0, n_det // 3, n_det], np.int32)
    flag = rng.choice(np.array([de.IGNORED, de.TP, de.FP], np.int32), n_det)
    npos = np.array([max(1, n_det // 2), max(1, n_det // 4)][:n_cls], np.int32)
    pk = de.Packed(n_classes=n_cls, det_key=det_key, cls_off=cls_off, npos=npos)
    hcur = de.curve_arrays_host(pk, flag)
    names = ("perm", "cum_tp", "cum_fp", "rec", "prec", "ap_area", "ap_11pt")
    cur = dict((n, t.cpu().numpy()) for n, t in zip(names, ops.det_eval_curve(det_key, cls_off, flag, npos, device=DEV)))
    for name in ("perm", "cum_tp", "cum_fp"):
        assert np.array_equal(cur[name], hcur[name]), name
    for name in ("rec", "prec", "ap_area", "ap_11pt"):
        assert np.array_equal(_bits(cur[name]), _bits(hcur[name])), name


def test_two_runs_give_the_same_bits(fresh):
    from i2vsgg_amd import detection_eval as de
    a = de.evaluate_packed(fresh, 0.5, device=DEV)
    b = de.evaluate_packed(fresh, 0.5, device=DEV)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    for name in a[3]:
        assert a[3][name].tobytes() == b[3][name].tobytes(), name


def test_device_refuses_what_the_host_form_refuses():
    from i2vsgg_amd import _lib, ops
    z = np.zeros(0, np.int32)
    with pytest.raises(_lib.I2VError):                    # a table that points past the detections: a status, no fault
        ops.det_eval_match(np.array([0, 9], np.int32), np.array([0], np.int32), np.array([0, 0], np.int32), np.zeros(4, np.int32),
                           np.zeros((4, 4)), np.zeros((0, 4)), z, device=DEV)
    with pytest.raises(_lib.I2VError):
        ops.det_eval_curve(np.zeros(4, np.int32), np.array([0, 2, 9], np.int32), np.zeros(4, np.int32), np.array([1, 1], np.int32),
                           device=DEV)
    with pytest.raises(_lib.I2VError):
        ops.det_eval_curve(np.zeros(4, np.int32), np.array([0, 2], np.int32), np.zeros(4, np.int32), np.array([1], np.int32), device=DEV)


def test_imdb_hook_on_detect_step_output_device_equals_host(tmp_path, capsys):
    """test_instance_styled.py on a synthetic imdb (random weights, the captured DetectStep, 3 frames per replay): its
    evaluate_detections hook fires on the GPU; the same call on the host gives the same result."""
    import test_instance_styled as td
    from i2vsgg_amd.model.utils import config as c
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    saved = copy.deepcopy(dict(c.cfg))
    try:
        all_boxes = td.main(["--frames", "3", "--output_dir", str(tmp_path / "o"), "--imdbval_name", "synthetic_10_v", "--scale", "192",
                             "--set", "TEST.RPN_POST_NMS_TOP_N", "64"])
    finally:
        c._merge_a_into_b(c.AttrDict(saved), c.cfg)
    out = capsys.readouterr().out
    assert "Mean AP = " in out and (tmp_path / "o" / "res101" / "synthetic" / "detection_eval.json").exists()
    assert sum(len(all_boxes[j][i]) for j in range(1, 16) for i in range(10)) > 0
    imdb = get_imdb("synthetic_10_v")
    dev = imdb.evaluate_detections(all_boxes, str(tmp_path / "d"), device=DEV)
    host = imdb.evaluate_detections(all_boxes, str(tmp_path / "h"), device=None)
    assert _same_doubles(dev["aps"], host["aps"]) and _same_doubles(dev["mean_ap"], host["mean_ap"])
    assert _same_doubles(dev["mean_ap_present"], host["mean_ap_present"])
    for name in imdb.classes[1:]:
        assert _same_doubles(dev["rec"][name], host["rec"][name]) and _same_doubles(dev["prec"][name], host["prec"][name]), name
