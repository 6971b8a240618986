#!/usr/bin/env python3
"""The detection test loop of ``test_instance_styled.py`` with the RPN's proposals kept: ONE pass over the test roidb writes
``detections.pkl`` as that script does and, next to it, ``proposals.pkl``, and prints the proposals' recall and average recall.

Flags, data path, network, checkpoint layout and schedule are that script's (its own ``parse_args`` reads them; frames grouped
by size, ``--frames`` per replayed graph, short groups at the end, ``--device_prep``); the per-frame body is the same
``eval.detect_frame`` / ``eval.DetectStep``, built with ``keep_proposals=True``.  Per image the proposals are divided by the image's
scale in float64, the division the reference's test loop applies to its boxes (test_net_instance_styleD_bilinear.py:171):
``proposals[i] = float64(rois) / float64(im_info[i][2])``, an (n, 4) array, best first.  They are scored on the GPU
(``i2vsgg_amd.proposal_eval``: recall at IoU 0.5 ... 0.95 and AR per candidate budget and object size; ``--limits`` / ``--areas``
as in ``eval_proposals.py``, which scores either written file again)."""
import argparse
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse_args(argv=None):
    """(the detection test loop's arguments, limits, areas): the flags of this script are taken out first -- ``--limits``, ``--areas``
    and ``--soft_nms {off,linear,gaussian}`` [``--soft_nms_sigma`` 0.5] [``--soft_nms_min_score`` 0.001]: Soft-NMS per class in the
    post-processing (i2vsgg_amd/soft_nms.py, Nt = cfg.TEST.NMS) instead of the reference's NMS; default off.  The returned
    namespace carries ``soft_nms``, the keyword of ``eval.detect_frame`` / ``eval.DetectStep``."""
    import test_instance_styled as td
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--limits", nargs="+", type=lambda t: None if t == "all" else int(t), default=None)
    p.add_argument("--areas", nargs="+", default=None)
    p.add_argument("--soft_nms", default="off", choices=["off", "linear", "gaussian"])
    p.add_argument("--soft_nms_sigma", type=float, default=0.5)
    p.add_argument("--soft_nms_min_score", type=float, default=0.001)
    own, rest = p.parse_known_args(argv)
    a = td.parse_args(rest)
    a.soft_nms = None if own.soft_nms == "off" else (own.soft_nms, own.soft_nms_sigma, own.soft_nms_min_score)
    return a, own.limits, own.areas


def main(argv=None):
    a, limits, areas = parse_args(argv)
    from i2vsgg_amd import eval as ev, proposal_eval, train
    from i2vsgg_amd.model.faster_rcnn.layers import load_reference_state
    from i2vsgg_amd.model.utils import config as c
    from i2vsgg_amd.roi_data_layer.roibatchLoader import roibatchLoader
    from i2vsgg_amd.roi_data_layer.roidb import combined_roidb
    dev = torch.device("cuda:0")
    c.cfg_from_file(c.default_cfg_file(a.net))
    c.cfg_from_list(["ANCHOR_SCALES", "[8, 16, 32]", "ANCHOR_RATIOS", "[0.5,1,2]", "MAX_NUM_GT_BOXES", "30"])   # parser_func.py:198-199
    if a.scale:
        c.cfg_from_list(["TEST.SCALES", "(%d,)" % a.scale, "TRAIN.SCALES", "(%d,)" % a.scale])
    if a.set_cfgs:
        c.cfg_from_list(a.set_cfgs)
    np.random.seed(c.cfg.RNG_SEED)
    c.cfg.TRAIN.USE_FLIPPED = False
    imdb, roidb, ratio_list, ratio_index = combined_roidb(a.imdbval_name, False)
    if hasattr(imdb, "competition_mode"):
        imdb.competition_mode(on=True)
    print("%d roidb entries" % len(roidb))
    net = train.build_instance_styled_net(101 if a.net == "res101" else 50, n_cls=imdb.num_classes, device=dev, ic=a.ic, gc=a.gc,
                                          class_agnostic=a.class_agnostic)
    if a.load_name:
        ck = torch.load(a.load_name, map_location="cpu")
        load_reference_state(net, ck["model"], strict=False)
        if "pooling_mode" in ck:
            c.cfg.POOLING_MODE = ck["pooling_mode"]
        print("load checkpoint %s" % a.load_name)
    net.eval()

    num_images = len(roidb)
    all_boxes = [[[] for _ in range(num_images)] for _ in range(imdb.num_classes)]
    proposals = [None] * num_images
    empty = np.zeros((0, 5), np.float32)
    u8 = a.device_prep and a.frames > 1
    dataset = roibatchLoader(roidb, ratio_list, ratio_index, 1, imdb.num_classes, training=False, normalize=False, device_prep=u8)
    loader = torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False, num_workers=a.num_workers, pin_memory=True)

    def keep(i, per_class, rois, scale):
        for j in range(1, imdb.num_classes):
            all_boxes[j][i] = per_class[j] if len(per_class[j]) else empty
        proposals[i] = rois.astype(np.float64) / np.float64(scale)

    t0 = time.time()
    if a.frames <= 1:
        z, nb = torch.zeros(1, 1, 5, device=dev), torch.zeros(1, device=dev)
        for i, data in enumerate(loader):
            per_class, rois = ev.detect_frame(net, data[0].to(dev), data[1].to(dev), z, nb, thresh=a.thresh, max_per_image=a.max_per_image,
                                              class_agnostic=a.class_agnostic, keep_proposals=True, soft_nms=a.soft_nms)
            keep(i, per_class, rois, data[1].reshape(-1)[2].item())
    else:
        step = ev.DetectStep(net, frames=a.frames, thresh=a.thresh, max_per_image=a.max_per_image, class_agnostic=a.class_agnostic,
                             device=dev, use_graph=not a.no_graph, keep_proposals=True, soft_nms=a.soft_nms)
        groups, order = {}, []

        def pack(g):
            # (image index, the scale as im_info holds it: row [h, w, scale], or the u8 meta row [flipped, h, w, scale, target])
            order.append([(t[0], float(np.float32(t[2].reshape(-1)[3 if u8 else 2].item()))) for t in g])
            if u8:
                return [t[1] for t in g], torch.cat([t[2] for t in g])
            return torch.cat([t[1] for t in g]), torch.cat([t[2] for t in g])

        def batches():
            # frames of one (resized) size travel together; a group leaves when it is full, the rest at the end
            for i, data in enumerate(loader):
                size = (int(data[1][0][1]), int(data[1][0][2])) if u8 else tuple(data[0].shape[2:])
                g = groups.setdefault(size, [])
                g.append((i, data[0], data[1]))
                if len(g) == a.frames:
                    yield pack(g)
                    g.clear()
            for g in groups.values():
                if g:
                    yield pack(g)

        for k, (res, props) in enumerate(step.run(batches(), u8=u8)):
            for (i, scale), per_class, rois in zip(order[k], res, props):
                keep(i, per_class, rois, scale)
    dt = time.time() - t0
    print("im_detect: %d images, %.2f ms per image (%.1f frames/s)" % (num_images, 1e3 * dt / max(num_images, 1), num_images / max(dt, 1e-9)))
    out_dir = os.path.join(a.output_dir, a.net, a.dataset)
    os.makedirs(out_dir, exist_ok=True)
    for name, obj in (("detections.pkl", all_boxes), ("proposals.pkl", proposals)):
        with open(os.path.join(out_dir, name), "wb") as f:
            pickle.dump(obj, f, pickle.HIGHEST_PROTOCOL)
        print("wrote %s" % os.path.join(out_dir, name))
    if hasattr(imdb, "evaluate_detections"):
        imdb.evaluate_detections(all_boxes, out_dir)
    res = proposal_eval.evaluate(proposals, roidb, limits or proposal_eval.DEFAULT_LIMITS, areas or proposal_eval.DEFAULT_AREAS,
                                 device=dev, num_classes=imdb.num_classes)
    proposal_eval.report(res)
    return all_boxes, proposals, res


if __name__ == "__main__":
    main()
