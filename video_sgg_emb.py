#!/usr/bin/env python3
"""Relation test loop up to the video level (test_net_SGG_emb.py:196-211 and :308-313): the per-frame part is
``test_sgg_emb.py``'s, unchanged (same flags, same ``relations.pkl``); its top-100 triplets per frame are then linked into video
relation instances on the GPU (``i2vsgg_amd.video.associate``) and written to ``video_relations.json`` beside ``relations.pkl``,
the file ``eval_video_relations.py`` scores.  ``--relations FILE`` skips the frame loop and starts from a pickle that an earlier
run wrote.  The synthetic imdb has no video ids: ``--frames_per_video N`` takes the frames in the order of their paths (the
loader's order depends on the frames' aspect ratios) and makes every N consecutive ones a video, numbered from 0 (default: the
whole imdb is one video, frame number = index).  Every other argument goes to ``test_sgg_emb.py``."""
import argparse
import json
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


def main(argv=None):
    p = argparse.ArgumentParser(description="Relation test loop + frame-to-video association on MI355X", add_help=False)
    p.add_argument("--frames_per_video", type=int, default=0)
    p.add_argument("--relations", default="", help="relations.pkl of an earlier run (skips the frame loop)")
    p.add_argument("--cpu", action="store_true", help="host implementation of the association")
    a, rest = p.parse_known_args(argv)
    import test_sgg_emb as frames
    from i2vsgg_amd import video
    if a.relations:
        with open(a.relations, "rb") as f:
            results = pickle.load(f)
        out_dir = os.path.dirname(os.path.abspath(a.relations))
    else:
        b = frames.parse_args(rest)
        results = frames.main(rest)
        out_dir = os.path.join(b.output_dir, b.net, b.dataset)
    paths, per = sorted(results), a.frames_per_video if a.frames_per_video > 0 else max(len(results), 1)
    index = dict((path, (str(k // per), k % per)) for k, path in enumerate(paths))
    t0 = time.time()
    relations = video.associate(video.from_frame_results(results, index), device=None if a.cpu else "cuda:0")
    out = os.path.join(out_dir, "video_relations.json")
    with open(out, "w") as f:
        json.dump(relations, f)
    print("association: %d videos, %d relations, %.1f ms; wrote %s" % (
        len(relations), sum(len(r) for r in relations.values()), 1e3 * (time.time() - t0), out))
    return relations


if __name__ == "__main__":
    main()
