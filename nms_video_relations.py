#!/usr/bin/env python3
"""Suppress duplicate video relations by trajectory vIoU (``i2vsgg_amd.video.suppress``, which states the rules): of two
relations of one video and triplet whose subject AND object trajectories overlap by more than ``--viou``, the better-scoring one
stays.  Input and output are JSON in the layout of ``video_relations.json`` ({video id: [{triplet, score, duration [fstart,
fend), sub_traj, obj_traj, ...}, ...]}); further keys of a relation pass through.  Per video the ``--pool`` best relations are
candidates and the first ``--max_per_video`` kept ones, in descending score, are written.  A file that ``video_sgg_emb.py`` wrote
without ``--rel_nms`` is already cut to 200 per video: duplicates that filled those slots go, what they displaced does not come
back.  The overlaps run on the GPU; ``--cpu`` runs the same rules on the host."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


def main(argv=None):
    p = argparse.ArgumentParser(description="NMS of video relations by trajectory vIoU")
    p.add_argument("--prediction", required=True)
    p.add_argument("--out", required=True)
    p.add_argument("--viou", type=float, required=True, help="threshold T in [0, 1]: ov > T suppresses")
    p.add_argument("--max_per_video", type=int, default=200)
    p.add_argument("--pool", type=int, default=2048, help="candidates per video, at most 4096")
    p.add_argument("--cpu", action="store_true", help="host implementation (no GPU needed)")
    a = p.parse_args(argv)
    from i2vsgg_amd import video
    with open(a.prediction) as f:
        prediction = json.load(f)
    try:
        relations, info = video.suppress(prediction, a.viou, a.max_per_video, a.pool, device=None if a.cpu else "cuda:0")
    except ValueError as e:
        raise SystemExit(str(e))
    with open(a.out, "w") as f:
        json.dump(relations, f)
    print(video.nms_totals(info) + " (vIoU %g); wrote %s" % (a.viou, a.out))
    return relations, info


if __name__ == "__main__":
    main()
