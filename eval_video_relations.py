#!/usr/bin/env python3
"""Score video relations against annotations (the ``evaluate`` call that ends test_net_SGG_emb.py): detection mean AP,
recall@50 / @100 and tagging precision@1 / 5 / 10.  Both files are JSON, {video id: [{triplet, score (predictions only),
duration [fstart, fend), sub_traj, obj_traj}, ...]}; ``video_sgg_emb.py`` writes the prediction file.  The trajectory
overlaps and the matching run on the GPU; ``--cpu`` runs the same rules on the host.  ``--rel_nms T`` first suppresses duplicate
relations of the prediction by trajectory vIoU (``i2vsgg_amd.video.suppress``)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


def main(argv=None):
    p = argparse.ArgumentParser(description="VidVRD detection / tagging metrics of video relations")
    p.add_argument("--prediction", required=True)
    p.add_argument("--groundtruth", required=True)
    p.add_argument("--viou_threshold", type=float, default=0.5)
    p.add_argument("--cpu", action="store_true", help="host implementation (no GPU needed)")
    p.add_argument("--rel_nms", type=float, default=None, help="suppress duplicate relations of the loaded prediction at this vIoU "
                   "before scoring (video.suppress at its defaults: 2048 candidates, 200 kept per video)")
    a = p.parse_args(argv)
    from i2vsgg_amd import video
    with open(a.prediction) as f:
        prediction = json.load(f)
    with open(a.groundtruth) as f:
        groundtruth = json.load(f)
    print("Number of videos in ground truth: %d" % len(groundtruth))
    print("Number of videos in prediction: %d" % len(prediction))
    if a.rel_nms is not None:
        prediction, info = video.suppress(prediction, a.rel_nms, device=None if a.cpu else "cuda:0")
        print(video.nms_totals(info) + " (vIoU %g)" % a.rel_nms)
    mean_ap, rec, mprec = video.evaluate(prediction, groundtruth, a.viou_threshold, device=None if a.cpu else "cuda:0")
    print("detection mean AP (used in challenge): {}".format(mean_ap))
    print("detection recall@50: {}".format(rec[50]))
    print("detection recall@100: {}".format(rec[100]))
    print("tagging precision@1: {}".format(mprec[1]))
    print("tagging precision@5: {}".format(mprec[5]))
    print("tagging precision@10: {}".format(mprec[10]))
    return mean_ap, rec, mprec


if __name__ == "__main__":
    main()
