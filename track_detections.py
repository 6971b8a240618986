#!/usr/bin/env python3
"""Link pickled detections into object tracks (Seq-NMS, ``i2vsgg_amd.seqnms``): the stage between the detector test loop and
the relation test loop.  ``--detections`` is the ``detections.pkl`` that ``test_instance_styled.py`` writes,
``all_boxes[class][image]``; ``--imdbval_name`` names the imdb it was run on.  Two files are written beside it (or into
``--output_dir``): ``detections_seqnms.pkl``, the rescored survivors in the same layout (``eval_detections.py`` reads it), and
``tracked_boxes.pkl``, {frame file name: {boxes, box_classes, scores, tids, rels: []}}, which ``test_sgg_emb.py`` /
``video_sgg_emb.py`` take as ``--target_gt_rels_path``.  Frames map to (video, frame number) as in ``video_sgg_emb.py``: the
frames in the order of their paths, every ``--frames_per_video`` consecutive ones a video (default: one video).  The linking
runs on the GPU; ``--cpu`` runs the same rules on the host.  ``--save_tracks`` also writes ``tracks.json``, the tracks as
trajectories, and ``--groundtruth FILE`` scores them right away (trajectory mAP, ``eval_tracks.py`` has the file formats); without
the two options nothing else is written or printed.  ``--stitch_gap G`` (default 0: off, every file is what it was) adds the
stitching step (``seqnms.stitch_arrays_host`` has the rules): tracklets are joined across up to G missed frames where the boxes
overlap by ``--stitch_iou``, both pickles carry the interpolated boxes (``tracked_boxes.pkl`` marks them under ``"interp"``),
``tracks.json`` and ``--groundtruth`` see the stitched tracks, and one more line reports the links made and the boxes added."""
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
    p = argparse.ArgumentParser(description="Seq-NMS over pickled detections")
    p.add_argument("--detections", required=True)
    p.add_argument("--imdbval_name", required=True)
    p.add_argument("--frames_per_video", type=int, default=0)
    p.add_argument("--link_iou", type=float, default=0.5)
    p.add_argument("--nms_iou", type=float, default=0.3)
    p.add_argument("--rescore", default="avg", choices=["avg", "max"])
    p.add_argument("--score_thresh", type=float, default=0.0, help="detections below it take no part")
    p.add_argument("--min_score", type=float, default=0.7, help="tracked_boxes.pkl: a box needs a new score above it")
    p.add_argument("--max_per_class", type=int, default=10, help="tracked_boxes.pkl: boxes per frame and class")
    p.add_argument("--min_len", type=int, default=1, help="tracked_boxes.pkl: members a track needs")
    p.add_argument("--stitch_gap", type=int, default=0, help="join tracklets across up to this many missed frames (1..7) and "
                   "interpolate the missed boxes; 0: off")
    p.add_argument("--stitch_iou", type=float, default=0.3, help="with --stitch_gap: the overlap a tracklet's end box and the next "
                   "one's start box need")
    p.add_argument("--cpu", action="store_true", help="host implementation (no GPU needed)")
    p.add_argument("--output_dir", default=None)
    p.add_argument("--save_tracks", action="store_true", help="also write tracks.json: the tracks as trajectories (eval_tracks.py reads it)")
    p.add_argument("--groundtruth", default=None, help="annotated trajectories (.json) or per-frame boxes with tids (.pkl): "
                   "print the trajectory mAP of the tracks right after linking (i2vsgg_amd/track_eval.py)")
    p.add_argument("--thresholds", nargs="+", type=float, default=[0.5, 0.7, 0.9], help="with --groundtruth: the vIoU thresholds")
    a = p.parse_args(argv)
    from i2vsgg_amd import seqnms
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    with open(a.detections, "rb") as f:
        all_boxes = pickle.load(f)
    imdb = get_imdb(a.imdbval_name)
    n = len(all_boxes[0]) if len(all_boxes) else 0
    paths = [imdb.image_path_at(i) for i in range(n)]
    index = seqnms.frame_index_of_paths(paths, a.frames_per_video)
    frame_index = [index[path] for path in paths]
    t0 = time.time()
    interp, stitched = None, {}
    if a.stitch_gap:
        out, tracks, interp = seqnms.seq_nms_stitched(all_boxes, frame_index, a.link_iou, a.nms_iou, a.rescore, a.score_thresh,
                                                      a.stitch_gap, a.stitch_iou, device=None if a.cpu else "cuda:0", stats=stitched)
    else:
        out, tracks = seqnms.seq_nms(all_boxes, frame_index, a.link_iou, a.nms_iou, a.rescore, a.score_thresh,
                                     device=None if a.cpu else "cuda:0")
    dt = time.time() - t0
    anno = seqnms.to_annotations(out, tracks, [path.split("/")[-1] for path in paths], a.min_score, a.max_per_class, a.min_len,
                                 frame_index, interp=interp)
    count = lambda ab: sum(len(c) for row in ab[1:] for c in row)
    n_tracks = sum(len(set((frame_index[i][0], int(t)) for i in range(n) for t in tracks[j][i])) for j in range(len(tracks)))
    print("seq-nms: %d videos, %d classes, %d detections -> %d on %d tracks, %.1f ms; %d boxes for the relation loop" % (
        len(set(v for v, _ in frame_index)), max(len(all_boxes) - 1, 0), count(all_boxes), count(out), n_tracks, 1e3 * dt,
        sum(len(e["boxes"]) for e in anno.values())))
    if a.stitch_gap:
        print("stitch: %d links over at most %d missed frames (overlap >= %g), %d boxes added" % (
            stitched["links"], a.stitch_gap, a.stitch_iou, stitched["added"]))
    out_dir = a.output_dir or os.path.dirname(os.path.abspath(a.detections))
    os.makedirs(out_dir, exist_ok=True)
    for name, obj in (("detections_seqnms.pkl", out), ("tracked_boxes.pkl", anno)):
        with open(os.path.join(out_dir, name), "wb") as f:
            pickle.dump(obj, f, pickle.HIGHEST_PROTOCOL)
        print("wrote %s" % os.path.join(out_dir, name))
    if a.save_tracks or a.groundtruth:
        from i2vsgg_amd import track_eval
        trajs = track_eval.from_seq_nms(out, tracks, frame_index, a.min_len)
        if a.save_tracks:
            with open(os.path.join(out_dir, "tracks.json"), "w") as f:
                json.dump(trajs, f)
            print("wrote %s" % os.path.join(out_dir, "tracks.json"))
        if a.groundtruth:
            import eval_tracks
            gts = eval_tracks.load_groundtruth(a.groundtruth, dict((path.split("/")[-1], v) for path, v in index.items()))
            track_eval.report(track_eval.evaluate(trajs, gts, a.thresholds))       # host code, with or without --cpu
    return out, tracks, anno


if __name__ == "__main__":
    main()
