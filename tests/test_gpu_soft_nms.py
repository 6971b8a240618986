"""Soft-NMS on the device (csrc/soft_nms.hip through ops.soft_nms, ops.detection_postprocess(soft_nms=...), eval.DetectStep,
proposals_instance_styled.py --soft_nms) against the host form of i2vsgg_amd/soft_nms.py under its exactness rules: hard and linear
bit for bit in rows, order and scores; gaussian in rows and order, each score within d * 2^-23 of the host's for a row that
received d decays (the float64 exp may differ in its last bit).  The cases and the host form's answers come from
tests/soft_nms_cases.py; that every gaussian case keeps the margin which makes the order comparison meaningful is asserted on the
CPU (tests/test_soft_nms_host.py).  Needs a real MI355X: `pytest -m gpu`."""
import copy
import pickle

import numpy as np
import pytest
import torch

import soft_nms_cases as sc
from conftest import record_margin
from i2vsgg_amd import soft_nms as sn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from i2vsgg_amd import ops as o
    return o


@pytest.fixture()
def keep_cfg():
    """The global cfg singleton is put back afterwards."""
    from i2vsgg_amd.model.utils import config as c
    saved = copy.deepcopy(dict(c.cfg))
    yield c
    c._merge_a_into_b(c.AttrDict(saved), c.cfg)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _check_set(got_rows, got_src, case, method, what):
    """One set against the host form.  Returns the largest |ds| / (d 2^-23 s) seen (gaussian; 0 otherwise)."""
    assert np.array_equal(got_src, case.src), what
    assert np.array_equal(_bits(got_rows[:, :4]), _bits(case.out[:, :4])), what
    if method != "gaussian":
        assert np.array_equal(_bits(got_rows[:, 4]), _bits(case.out[:, 4])), what
        return 0.0
    s_dev, s_host, d = got_rows[:, 4].astype(np.float64), case.out[:, 4].astype(np.float64), case.decays.astype(np.float64)
    exact = d == 0
    assert np.array_equal(_bits(got_rows[exact, 4]), _bits(case.out[exact, 4])), what
    err = np.abs(s_dev - s_host)
    assert (err <= d * 2.0 ** -23 * np.abs(s_host)).all(), (what, float((err[~exact] / (d[~exact] * 2.0 ** -23 * np.abs(s_host[~exact]))).max()))
    return float((err[~exact] / (d[~exact] * 2.0 ** -23 * np.abs(s_host[~exact]))).max()) if (~exact).any() else 0.0


@pytest.mark.parametrize("method", sn.METHODS)
@pytest.mark.parametrize("n", sc.SIZES)
def test_soft_nms_equals_the_host_form(ops, n, method):
    worst = 0.0
    for batch in sc.batches(n, method):
        dets, counts = sc.pack(batch, n)
        out, src, num = ops.soft_nms(torch.from_numpy(dets).to(DEV), torch.from_numpy(counts).to(DEV), method, sc.NT, sc.SIGMA,
                                     sc.MIN_SCORE)
        out, src, num = out.cpu().numpy(), src.cpu().numpy(), num.cpu().numpy()
        assert num.tolist() == [c.num for c in batch], [(c.family, len(c.rows)) for c in batch]
        for i, c in enumerate(batch):
            worst = max(worst, _check_set(out[i, :num[i]], src[i, :num[i]], c, method, (c.family, n, len(c.rows), method)))
    if method == "gaussian":
        print("gaussian n=%d: largest |ds| / (d 2^-23 s) = %.4f" % (n, worst))
        record_margin("test_soft_nms_equals_the_host_form", "gaussian n=%d |ds| / (d 2^-23 s)" % n, worst, 1.0)


def test_counts_none_takes_every_row_and_a_2d_input_is_one_set(ops):
    c = sc.case("random", 128, 128, "linear")
    out, src, num = ops.soft_nms(torch.from_numpy(np.array(c.rows)).to(DEV), None, "linear", sc.NT)
    assert out.shape == (1, 128, 5) and int(num[0]) == c.num
    _check_set(out[0, :c.num].cpu().numpy(), src[0, :c.num].cpu().numpy(), c, "linear", "2d")


def test_more_than_4096_rows_is_an_argument_error(ops):
    """An argument check: nothing is launched."""
    from i2vsgg_amd._lib import I2VError
    dets = torch.zeros((1, 4097, 5), device=DEV)
    with pytest.raises(I2VError, match=r"\(-1\): soft_nms: at most 4096 rows per set"):
        ops.soft_nms(dets, None, "linear", 0.3)
    with pytest.raises(ValueError):
        ops.soft_nms(dets[:, :8], None, "quadratic", 0.3)


def test_the_largest_set_4096_rows(ops):
    """The capacity itself (16 waves, four rows per lane, 64 KiB of boxes in LDS), hard and linear, bit for bit: half the rows
    clustered, half filler that overlaps nothing, so the loop makes more than 2048 picks."""
    rows = sc.build_rows("random", 4096, 2048, 4242)
    for method in ("hard", "linear"):
        want, wsrc, wnum = sn.soft_nms_host(rows, None, method, sc.NT)
        out, src, num = ops.soft_nms(torch.from_numpy(rows).to(DEV), None, method, sc.NT)
        k = int(wnum[0])
        assert k > 2048
        assert int(num[0]) == k and np.array_equal(src[0, :k].cpu().numpy(), wsrc[0, :k])
        assert np.array_equal(_bits(out[0, :k].cpu().numpy()), _bits(want[0, :k]))


def test_gaussian_at_the_capacity(ops):
    """The 16-wave, four-rows-per-lane gaussian kernel: 4096 valid rows, more than 4000 picks, decaying rows in the first, the
    middle and the last registers (soft_nms_cases.banded_gaussian_case; its margin is asserted on the CPU)."""
    c = sc.banded_gaussian_case()
    out, src, num = ops.soft_nms(torch.from_numpy(np.array(c.rows)).to(DEV), None, "gaussian", sc.NT, sc.SIGMA, sc.MIN_SCORE)
    assert int(num[0]) == c.num
    worst = _check_set(out[0, :c.num].cpu().numpy(), src[0, :c.num].cpu().numpy(), c, "gaussian", "banded 4096")
    print("gaussian n=4096: largest |ds| / (d 2^-23 s) = %.4f" % worst)
    record_margin("test_gaussian_at_the_capacity", "gaussian n=4096 |ds| / (d 2^-23 s)", worst, 1.0)


# ------------------------------------------------------------------------------------------------ detection post-processing
R_DET, C_DET = 40, 5


def _detection_inputs():
    """rois / cls_prob / bbox_pred of 40 rois in five clusters, so that rois of a class overlap; every score distinct."""
    rng = np.random.default_rng(515)
    c = rng.uniform([40, 40], [400, 240], (5, 2))
    pick = rng.integers(0, 5, R_DET)
    xy = c[pick] + rng.normal(0, 6.0, (R_DET, 2))
    wh = rng.uniform(40, 90, (5, 2))[pick] + rng.normal(0, 4.0, (R_DET, 2))
    rois = np.zeros((R_DET, 5), F32)
    rois[:, 1:3], rois[:, 3:5] = xy, xy + wh
    prob = rng.uniform(0.02, 1.0, (R_DET, C_DET)).astype(F32)
    prob /= prob.sum(1, keepdims=True)
    pred = rng.normal(0, 0.05, (R_DET, 4 * C_DET)).astype(F32)
    assert len(np.unique(prob)) == prob.size
    return rois, prob, pred, (320.0, 480.0, 1.25)


@pytest.mark.parametrize("method", ("linear", "gaussian", "hard"))
def test_detection_postprocess_soft_equals_the_composed_expectation(ops, method):
    """The expectation is composed without the new code: today's hard entry at nms_thresh 1.0, max_per_image 0 (nothing can be
    suppressed or cut) gives the decoded, thresholded, sorted rows of every class; postprocess_host does the rest."""
    rois, prob, pred, (h, w, s) = _detection_inputs()
    t = [torch.from_numpy(a).to(DEV) for a in (rois, prob, pred)]
    thresh = 0.05
    dets, counts = ops.detection_postprocess(*t, h, w, s, score_thresh=thresh, nms_thresh=1.0, max_per_image=0)
    dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    assert counts[0] == 0 and counts[1:].min() >= 8 and counts.tolist() == [0] + [(prob[:, j] > thresh).sum() for j in range(1, C_DET)]
    opt = (method, 0.5, 0.001)
    info = torch.tensor([h, w, s], device=DEV)
    stats = {}
    full, nfull = sn.postprocess_host(dets, counts, method, 0.3, max_per_image=0, stats=stats)
    decays = stats["decays"]
    if method == "gaussian":                                # the case is fit for the order comparison, within a class and at the cut
        assert sc.fit(stats, R_DET), stats
        every = np.sort(np.concatenate([full[j, :nfull[j], 4] for j in range(C_DET)]).astype(np.float64))
        assert (np.diff(every) / every[1:]).min() > sn.margin(R_DET)
    survivors = int(nfull.sum())
    cut = survivors // 2
    for max_per_image in (0, survivors + 1, cut):
        want, wnum = sn.postprocess_host(dets, counts, method, 0.3, max_per_image=max_per_image)
        if max_per_image == cut:                             # the cut bites, and on decayed scores
            assert wnum.sum() < survivors
        for kw in ({}, {"im_info": info}):
            g, gn = ops.detection_postprocess(*t, h, w, s, score_thresh=thresh, nms_thresh=0.3, max_per_image=max_per_image,
                                              soft_nms=opt, **kw)
            g, gn = g.cpu().numpy(), gn.cpu().numpy()
            assert gn.tolist() == wnum.tolist(), (method, max_per_image, kw.keys())
            for j in range(C_DET):
                a, b = g[j, :gn[j]], want[j, :wnum[j]]
                assert np.array_equal(_bits(a[:, :4]), _bits(b[:, :4])), (method, j)
                if method == "gaussian":
                    d = decays[j][:gn[j]]
                    assert (np.abs(a[:, 4].astype(np.float64) - b[:, 4]) <= d * 2.0 ** -23 * np.abs(b[:, 4])).all(), (method, j)
                else:
                    assert np.array_equal(_bits(a[:, 4]), _bits(b[:, 4])), (method, j)
    # soft decays where hard deletes: more rows than today's path at the same threshold, and decayed scores among them
    hard, hn = ops.detection_postprocess(*t, h, w, s, score_thresh=thresh, nms_thresh=0.3, max_per_image=0)
    if method != "hard":
        assert nfull.sum() > int(hn.sum())
    else:
        assert nfull.tolist() == hn.cpu().tolist()
        for j in range(C_DET):
            assert np.array_equal(_bits(full[j, :nfull[j]]), _bits(hard[j, :nfull[j]].cpu().numpy()))


def test_soft_nms_none_is_todays_call(ops):
    rois, prob, pred, (h, w, s) = _detection_inputs()
    t = [torch.from_numpy(a).to(DEV) for a in (rois, prob, pred)]
    info = torch.tensor([h, w, s], device=DEV)
    for kw in ({}, {"im_info": info}):
        outs = []
        for extra in ({}, {"soft_nms": None}, {"soft_nms": "off"}):
            out = (torch.full((C_DET, R_DET, 5), -7.0, device=DEV), torch.full((C_DET,), -7, device=DEV, dtype=torch.int32))
            ops.detection_postprocess(*t, h, w, s, score_thresh=0.05, out=out, **kw, **extra)
            outs.append((out[0].cpu().numpy().tobytes(), out[1].cpu().numpy().tobytes()))
        assert outs[0] == outs[1] == outs[2]


# ------------------------------------------------------------------------------------------------ the test loop
def test_detect_step_with_soft_nms_equals_frame_by_frame(keep_cfg):
    """DetectStep(soft_nms=linear) replayed as a graph == detect_frame(soft_nms=linear) frame by frame, on the network of
    test_gpu_models.test_detect_step_equals_frame_by_frame_eval; and both differ from the greedy NMS."""
    import i2vsgg_amd.synthetic as syn
    from i2vsgg_amd import eval as ev
    from i2vsgg_amd._lib import TUNE, lib
    from i2vsgg_amd.model.faster_rcnn.resnet_instance_styleD_bilinear import resnet
    c = keep_cfg
    c.cfg_from_file(c.default_cfg_file("res101"))
    c.cfg_from_list(["ANCHOR_SCALES", "[8, 16, 32]", "ANCHOR_RATIOS", "[0.5,1,2]", "MAX_NUM_GT_BOXES", "30"])
    torch.manual_seed(1)
    net = resnet(tuple(range(16)), 50)
    net.create_architecture()
    net.to(DEV).eval()
    ims = [torch.from_numpy(syn.frames(40 + i, 1, 320, 480)[0]).to(DEV) for i in range(3)]
    infos = [torch.tensor([[320.0, 480.0, s]], device=DEV) for s in (1.0, 1.6, 0.8)]
    z, nb = torch.zeros(1, 1, 5, device=DEV), torch.zeros(1, device=DEV)
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    try:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)        # no split-K atomics: two forwards of a frame are bit-equal
        want = [ev.detect_frame(net, im, info, z, nb, soft_nms="linear") for im, info in zip(ims, infos)]
        hard = ev.detect_frame(net, ims[0], infos[0], z, nb)
        step = ev.DetectStep(net, frames=2, device=DEV, soft_nms=("linear", 0.5, 0.001))
        got = step(torch.cat(ims[:2]), torch.cat(infos[:2])) + step(ims[2], infos[2])
        assert step.graph_error is None and step.shapes[step._staged].graph
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)
    assert len(got) == 3
    for f in range(3):
        assert len(got[f]) == 16
        for j in range(16):
            assert np.array_equal(got[f][j], want[f][j]), (f, j)
            assert (np.diff(want[f][j][:, 4]) <= 0).all()
    assert 0 < sum(len(x) for x in want[0]) <= 100
    assert any(not np.array_equal(a, b) for a, b in zip(want[0], hard))


def test_script_flag_writes_the_eager_form_and_differs_from_off(keep_cfg, tmp_path):
    """proposals_instance_styled.py --soft_nms linear (the detection test loop of test_instance_styled.py, same flags and the same
    detections.pkl, plus the proposals): the graph form's detections.pkl equals the frame-by-frame form and differs from the
    flag-off pickle (random weights: rois of a class overlap freely); off is the default, and with it off the file is the one
    test_instance_styled.py writes."""
    import proposals_instance_styled as ps
    import test_instance_styled as td
    from i2vsgg_amd._lib import TUNE, lib
    common = ["--net", "res50", "--imdbval_name", "synthetic_6_v", "--scale", "192", "--set", "TEST.RPN_POST_NMS_TOP_N", "64"]
    assert ps.parse_args([])[0].soft_nms is None and ps.parse_args(["--soft_nms", "off"])[0].soft_nms is None
    assert ps.parse_args(["--set", "TEST.NMS", "0.3", "--soft_nms", "gaussian", "--soft_nms_sigma", "0.25"])[0].soft_nms == ("gaussian", 0.25, 0.001)
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    res = {}
    try:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)
        for name, main, extra in (("eager", ps.main, ["--frames", "1", "--soft_nms", "linear"]),
                                  ("graph", ps.main, ["--frames", "3", "--soft_nms", "linear"]),
                                  ("off", ps.main, ["--frames", "3"]), ("off_flag", ps.main, ["--frames", "3", "--soft_nms", "off"]),
                                  ("plain", td.main, ["--frames", "3"])):
            torch.manual_seed(11)                            # the same random weights in every run
            out = main(extra + ["--output_dir", str(tmp_path / name)] + common)
            res[name] = out[0] if main is ps.main else out
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)
    pk = {}
    for name in res:
        with open(tmp_path / name / "res50" / "synthetic" / "detections.pkl", "rb") as f:
            raw = f.read()
        pk[name] = raw
        saved = pickle.loads(raw)
        assert len(saved) == 16 and len(saved[1]) == 6
        for j in range(1, 16):
            for i in range(6):
                assert np.array_equal(saved[j][i], res[name][j][i])
    n_det = 0
    for j in range(1, 16):
        for i in range(6):
            assert np.array_equal(res["graph"][j][i], res["eager"][j][i]), (j, i)
            n_det += len(res["graph"][j][i])
    assert n_det > 0
    assert pk["off"] == pk["off_flag"] == pk["plain"]
    assert pk["graph"] != pk["off"]
    assert any(not np.array_equal(res["graph"][j][i], res["off"][j][i]) for j in range(1, 16) for i in range(6))
