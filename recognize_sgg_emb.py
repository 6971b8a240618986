#!/usr/bin/env python3
"""Predicate recognition test loop (the ``pre_det`` branch of test_net_SGG_emb.py, :213-228 and :318-324) on the HIP path: the
loader of ``test_sgg_emb.py`` (same flags); per frame the backbone, the eval branch of ``forward_predicate`` on the frame's
annotated pairs and ``recognition_output`` (``eval.recognition_frame``; the loop is eager, one frame at a time).  The per-frame
scores go to ``<output_dir>/frame_recognitions.pkl`` as {video: {frame number: {sub_scores, obj_scores, pre_scores, tids} or {}}};
with a ground truth (``--groundtruth annotations.json``, VidVRD-style relations with subject_tid / object_tid / duration) the
scores are aligned with the annotated tracks and accuracy@1/5 is printed and written to ``recognition.json``
(``i2vsgg_amd.recognition``; on the GPU, ``--cpu``: the same rules on the host).  Frames become videos as in
``video_sgg_emb.py``: in the order of their paths, every ``--frames_per_video`` consecutive ones a video, numbered from 0.  A
synthetic imdb without ``--target_gt_rels_path`` gets the seeded recognition set of ``synthetic.recognition_set`` and its
ground truth."""
import argparse
import json
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser(description="Predicate recognition on MI355X", add_help=False)
    p.add_argument("--groundtruth", default="", help="video-level annotations (JSON)")
    p.add_argument("--predicates", default="", help="JSON list of predicate names (or {name: label}); default: labels only")
    p.add_argument("--frames_per_video", type=int, default=0)
    p.add_argument("--cpu", action="store_true", help="host implementation of the alignment and the metrics")
    b, rest = p.parse_known_args(argv)
    import test_sgg_emb as frames
    a = frames.parse_args(rest)
    from i2vsgg_amd import eval as ev, recognition, synthetic as syn, train
    from i2vsgg_amd.model.faster_rcnn.layers import load_reference_state
    from i2vsgg_amd.model.utils import config as c
    from i2vsgg_amd.roi_data_layer.roibatchLoader import roibatchLoader
    from i2vsgg_amd.roi_data_layer.roidb import SyntheticImdb, combined_roidb
    dev = torch.device("cuda:0")
    c.cfg_from_file(c.default_cfg_file(a.net))
    if a.scale:
        c.cfg_from_list(["TEST.SCALES", "(%d,)" % a.scale, "TRAIN.SCALES", "(%d,)" % a.scale])
    if a.set_cfgs:
        c.cfg_from_list(a.set_cfgs)
    np.random.seed(c.cfg.RNG_SEED)
    c.cfg.TRAIN.USE_FLIPPED = False
    imdb, roidb, ratio_list, ratio_index = combined_roidb(a.imdbval_name, False)
    print("%d roidb entries" % len(roidb))
    net = train.build_sgg_net(101 if a.net == "res101" else 50, a.num_relations, a.num_classes, device=dev)
    if a.load_name:
        load_reference_state(net, torch.load(a.load_name, map_location="cpu")["model"], strict=False)
        print("load checkpoint %s" % a.load_name)
    key = lambda path: path.split("/")[-1]                  # the annotation dicts are keyed by the frame's file name
    groundtruth = None
    if a.target_gt_rels_path:
        with open(a.target_gt_rels_path, "rb") as f:
            net.vrd.target_gt_rels = pickle.load(f, encoding="bytes")
    elif isinstance(imdb, SyntheticImdb):
        keys = [key(imdb.image_path_at(i)) for i in range(imdb.num_images)]
        net.vrd.target_gt_rels, groundtruth = syn.recognition_set(c.cfg.RNG_SEED, keys, imdb._sizes, b.frames_per_video,
                                                                  a.num_relations, a.num_classes, classes=imdb.classes)
    else:
        raise SystemExit("no relation annotations: pass --target_gt_rels_path")
    if b.groundtruth:
        with open(b.groundtruth) as f:
            groundtruth = json.load(f)
    net.eval()
    dataset = roibatchLoader(roidb, ratio_list, ratio_index, 1, imdb.num_classes, training=False, normalize=False)
    loader = torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False, num_workers=a.num_workers, pin_memory=True)
    results = {}
    t0 = time.time()
    for data in loader:                                      # test_net_SGG_emb.py:213-228
        path = data[4][0]
        sub, obj, pre, tids = ev.recognition_frame(net, data[0].to(dev), data[1].to(dev), key(path))
        results[path] = {} if sub is None else {"sub_scores": sub, "obj_scores": obj, "pre_scores": pre, "tids": tids}
    dt = time.time() - t0
    print("recognition scoring: %d frames, %d pairs, %.2f ms per frame" % (
        len(results), sum(len(r["tids"]) for r in results.values() if r), 1e3 * dt / max(len(results), 1)))
    paths, per = sorted(results), b.frames_per_video if b.frames_per_video > 0 else max(len(results), 1)
    frame_recognitions = {}
    for k, path in enumerate(paths):
        frame_recognitions.setdefault(str(k // per), {})[k % per] = results[path]
    out_dir = os.path.join(a.output_dir, a.net, a.dataset)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "frame_recognitions.pkl")
    with open(out, "wb") as f:
        pickle.dump(frame_recognitions, f, pickle.HIGHEST_PROTOCOL)
    print("wrote %s" % out)
    if groundtruth is None:
        return frame_recognitions, None
    predicates = recognition.predicate_names(b.predicates, a.num_relations)
    res = recognition.evaluate(frame_recognitions, groundtruth, list(imdb.classes), predicates, device=None if b.cpu else dev)
    recognition.report(res, imdb.classes)
    out = os.path.join(out_dir, "recognition.json")
    with open(out, "w") as f:
        json.dump({"metrics": recognition.to_json(res), "groundtruth": groundtruth, "classes": list(imdb.classes),
                   "predicates": predicates}, f)
    print("wrote %s" % out)
    return frame_recognitions, res


if __name__ == "__main__":
    main()
