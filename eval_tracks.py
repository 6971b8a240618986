#!/usr/bin/env python3
"""Trajectory mAP of object tracks against annotated trajectories (i2vsgg_amd/track_eval.py has the rules): per class and vIoU
threshold the average precision, their means, and the trajectory recall by length.  ``--tracks`` is the ``tracks.json`` that
``track_detections.py --save_tracks`` writes, {vid: [{category, score, frames, boxes}, ...]}.  ``--groundtruth`` is either a
``.json`` of the same layout (no scores) or a ``.pkl`` in the per-frame layout of annotated and tracked boxes, {frame file
name: {boxes, box_classes, tids, ...}}; its frames map to (video, frame number) as in ``track_detections.py``: with
``--imdbval_name`` the imdb's frames, else the pickle's own names, in the order of their paths, every ``--frames_per_video``
consecutive ones a video (default: one video).  The metric is host code (numpy) and needs no GPU; ``--cpu`` is accepted, as by
the other evaluation scripts, and changes nothing."""
import argparse
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


def load_groundtruth(path, index_by_name=None, frames_per_video=0):
    """{vid: [trajectory, ...]} from a ``.json`` of trajectories or a ``.pkl`` of per-frame boxes with tids.  ``index_by_name``
    {frame file name: (vid, fno)}; None: the pickle's own names in sorted order, ``frames_per_video`` to a video."""
    from i2vsgg_amd import seqnms, track_eval
    if path.endswith(".json"):
        with open(path) as f:
            return json.load(f)
    with open(path, "rb") as f:
        anno = pickle.load(f)
    if index_by_name is None:
        index_by_name = seqnms.frame_index_of_paths(list(anno), frames_per_video)
    return track_eval.from_frame_annotations(anno, index_by_name)


def main(argv=None):
    from i2vsgg_amd import seqnms, track_eval
    p = argparse.ArgumentParser(description="Trajectory mAP of object tracks")
    p.add_argument("--tracks", required=True, help="tracks.json of track_detections.py --save_tracks")
    p.add_argument("--groundtruth", required=True, help="trajectories (.json) or per-frame boxes with tids (.pkl)")
    p.add_argument("--imdbval_name", default=None, help="a .pkl ground truth: the imdb whose frames it annotates")
    p.add_argument("--frames_per_video", type=int, default=0)
    p.add_argument("--thresholds", nargs="+", type=float, default=list(track_eval.DEFAULT_THRESHOLDS))
    p.add_argument("--length_buckets", nargs="+", type=int, default=list(track_eval.DEFAULT_LENGTH_BUCKETS))
    p.add_argument("--cpu", action="store_true", help="accepted for symmetry: the metric always runs on the host")
    p.add_argument("--out", default=None, help="also write the result there as JSON (track_eval.json)")
    a = p.parse_args(argv)
    with open(a.tracks) as f:
        tracks = json.load(f)
    index = None
    if a.imdbval_name:
        from i2vsgg_amd.roi_data_layer.roidb import get_imdb
        imdb = get_imdb(a.imdbval_name)
        paths = [imdb.image_path_at(i) for i in range(len(imdb.roidb))]
        index = dict((path.split("/")[-1], v) for path, v in seqnms.frame_index_of_paths(paths, a.frames_per_video).items())
    gts = load_groundtruth(a.groundtruth, index, a.frames_per_video)
    res = track_eval.evaluate(tracks, gts, a.thresholds, a.length_buckets)
    track_eval.report(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
