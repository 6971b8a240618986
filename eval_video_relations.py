#!/usr/bin/env python3
"""Score video relations against annotations (the ``evaluate`` call that ends test_net_SGG_emb.py): detection mean AP,
recall@50 / @100 and tagging precision@1 / 5 / 10.  Both files are JSON, {video id: [{triplet, score (predictions only),
duration [fstart, fend), sub_traj, obj_traj}, ...]}; ``video_sgg_emb.py`` writes the prediction file.  The trajectory
overlaps and the matching run on the GPU; ``--cpu`` runs the same rules on the host."""
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
    a = p.parse_args(argv)
    from i2vsgg_amd import video
    with open(a.prediction) as f:
        prediction = json.load(f)
    with open(a.groundtruth) as f:
        groundtruth = json.load(f)
    print("Number of videos in ground truth: %d" % len(groundtruth))
    print("Number of videos in prediction: %d" % len(prediction))
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
