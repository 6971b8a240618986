#!/usr/bin/env python3
"""Relation test loop up to the video level (test_net_SGG_emb.py:196-211 and :308-313): the per-frame part is
``test_sgg_emb.py``'s, unchanged (same flags, same ``relations.pkl``); its top-100 triplets per frame are then linked into video
relation instances on the GPU (``i2vsgg_amd.video.associate``) and written to ``video_relations.json`` beside ``relations.pkl``,
the file ``eval_video_relations.py`` scores.  ``--associate tracks`` links along the track ids of the boxes the loop ran on
instead (``i2vsgg_amd.video.associate_tracks``; ``--max_gap G`` lets a relation miss up to G frames, ``--tracks FILE`` names the box
pickle, by default the loop's ``--target_gt_rels_path``).  ``--rel_nms T`` suppresses duplicate relations by trajectory vIoU before the cap of
200 (``i2vsgg_amd.video.suppress``; ``--rel_nms_pool N`` candidates per video).  ``--relations FILE`` skips the frame loop and starts from a pickle that an earlier
run wrote.  The synthetic imdb has no video ids: ``--frames_per_video N`` takes the frames in the order of their paths (the
loader's order depends on the frames' aspect ratios) and makes every N consecutive ones a video, numbered from 0 (default: the
whole imdb is one video, frame number = index).  ``--save_videofeat_path DIR`` adds the hand-off to the video-level stage
(lib/utils.py:100-132, called at test_net_SGG_emb.py:315): the frame loop keeps every pair's relation feature on the device, and
after the association ``i2vsgg_amd.relation_features`` pools one feature per relation in one kernel launch and writes
``DIR/<predicate>/<vid>_<pno>.npy``.  ``--save_feat_path DIR`` writes the predicate embeddings (``DIR/semantic_embedding.npy``,
:147-149) and, with ``--save_frame_feats``, ``DIR/<vid>/<fno>.npz`` (``pre_feat``, :171-182) per frame that had pairs.  The frame
loop's code does not know of this: it runs inside ``eval.keeping_relation_features``.  ``main(argv, hold={})`` leaves the device
store and the network in ``hold["arena"]`` / ``hold["net"]``.  Every other argument goes to ``test_sgg_emb.py``."""
import argparse
import json
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


NO_TRACKS = ("--associate tracks reads the track ids of the boxes the frame loop ran on: pass that pickle (tracked_boxes.pkl of "
             "track_detections.py) as --tracks, or as --target_gt_rels_path when the frame loop runs")


def main(argv=None, hold=None):
    p = argparse.ArgumentParser(description="Relation test loop + frame-to-video association on MI355X", add_help=False)
    p.add_argument("--frames_per_video", type=int, default=0)
    p.add_argument("--relations", default="", help="relations.pkl of an earlier run (skips the frame loop)")
    p.add_argument("--cpu", action="store_true", help="host implementation of the association (and of the feature pooling)")
    p.add_argument("--save_feat_path", default="", help="write DIR/semantic_embedding.npy (the predicate embeddings, "
                   "test_net_SGG_emb.py:147-149)")
    p.add_argument("--save_frame_feats", action="store_true", help="with --save_feat_path: also DIR/<vid>/<fno>.npz (pre_feat) per "
                   "frame that had pairs (test_net_SGG_emb.py:171-182), the input of pool_relation_features.py")
    p.add_argument("--save_videofeat_path", default="", help="write DIR/<predicate>/<vid>_<pno>.npy, one pooled relation "
                   "feature per video relation (lib/utils.py:100-132); the frame features stay on the device in between")
    p.add_argument("--feat_arena_mb", type=float, default=4096, help="largest device store of relation features, MiB")
    p.add_argument("--associate", choices=["boxes", "tracks"], default="boxes", help="boxes: the reference's association by box "
                   "overlap; tracks: along the track ids of the boxes the frame loop ran on (video.associate_tracks)")
    p.add_argument("--max_gap", type=int, default=0, help="with --associate tracks: frames (0..7) a relation may stay out of its "
                   "frames' top 100 and still go on")
    p.add_argument("--tracks", default="", help="with --associate tracks: the per-frame box pickle with tids (default: the frame "
                   "loop's --target_gt_rels_path; required with --relations)")
    p.add_argument("--rel_nms", type=float, default=None, help="suppress duplicate relations: of two relations of one triplet whose "
                   "subject and object trajectories both overlap by more than this vIoU the better one stays (video.suppress); the "
                   "association then keeps --rel_nms_pool candidates per video and the cap of 200 comes after the suppression")
    p.add_argument("--rel_nms_pool", type=int, default=0, help="with --rel_nms: candidates per video (default 2048, at most 4096)")
    a, rest = p.parse_known_args(argv)
    if a.rel_nms is None and a.rel_nms_pool:
        raise SystemExit("--rel_nms_pool belongs to --rel_nms: give it")
    if a.rel_nms is not None and not 0.0 <= a.rel_nms <= 1.0:
        raise SystemExit("--rel_nms lies in [0, 1] (got %r)" % a.rel_nms)
    if a.associate != "tracks" and (a.max_gap != 0 or a.tracks):
        raise SystemExit("--max_gap and --tracks belong to --associate tracks: give it")
    if a.associate == "tracks" and not 0 <= a.max_gap <= 7:
        raise SystemExit("--max_gap lies in 0..7 (got %d)" % a.max_gap)
    import test_sgg_emb as frames
    from i2vsgg_amd import video
    keep = bool(a.save_feat_path or a.save_videofeat_path)
    if a.save_frame_feats and not a.save_feat_path:
        raise SystemExit("--save_frame_feats writes under --save_feat_path: give it")
    sink = None
    if a.relations:
        if keep:
            raise SystemExit("--save_feat_path / --save_videofeat_path need the frame loop (the features live on the device during "
                             "the run); from files of an earlier run use pool_relation_features.py")
        if a.associate == "tracks" and not a.tracks:
            raise SystemExit(NO_TRACKS)
        with open(a.relations, "rb") as f:
            results = pickle.load(f)
        out_dir = os.path.dirname(os.path.abspath(a.relations))
    else:
        b = frames.parse_args(rest)
        a.tracks = a.tracks or b.target_gt_rels_path
        if a.associate == "tracks" and not a.tracks:     # before the frame loop runs for nothing
            raise SystemExit(NO_TRACKS)
        if keep:                                         # the loop's code is unchanged: the block makes its steps keep pre_feat
            from i2vsgg_amd import eval as ev, relation_features as rf
            with ev.keeping_relation_features(rf.ArenaSink("cuda:0", a.feat_arena_mb)) as sink:
                results = frames.main(rest)
        else:
            results = frames.main(rest)
        out_dir = os.path.join(b.output_dir, b.net, b.dataset)
    paths, per = sorted(results), a.frames_per_video if a.frames_per_video > 0 else max(len(results), 1)
    index = dict((path, (str(k // per), k % per)) for k, path in enumerate(paths))
    if sink is not None:
        if sink.arena is None:
            raise SystemExit("the frame loop ran no frame: there are no features to keep")
        sink.arena.rekey(dict((path.split("/")[-1], v) for path, v in index.items()))      # the loop keys a frame by its file name
        if hold is not None:
            hold["arena"], hold["net"] = sink.arena, sink.net
    if a.save_feat_path:
        os.makedirs(a.save_feat_path, exist_ok=True)
        import numpy as np
        np.save(os.path.join(a.save_feat_path, "semantic_embedding.npy"), rf.semantic_embedding(sink.net.vrd))
        n = rf.save_frame_feats(sink.arena, a.save_feat_path) if a.save_frame_feats else 0
        print("wrote %s/semantic_embedding.npy and the features of %d frames" % (a.save_feat_path, n))
    t0 = time.time()
    mode = ""
    pool = (a.rel_nms_pool or video.NMS_POOL) if a.rel_nms is not None else 0
    if pool and not 1 <= pool <= video.NMS_MAX_POOL:
        raise SystemExit("--rel_nms_pool lies in 1..%d (got %d)" % (video.NMS_MAX_POOL, pool))
    cap = dict(max_per_video=pool) if pool else {}       # with --rel_nms the suppression sees the candidates before the cap
    if a.associate == "tracks":
        with open(a.tracks, "rb") as f:
            tracks = pickle.load(f, encoding="bytes")
        relations = video.associate_tracks(video.from_frame_results(results, index, tracks), tracks, a.max_gap,
                                           device=None if a.cpu else "cuda:0", frame_to_video=index, **cap)
    else:
        relations = video.associate(video.from_frame_results(results, index), device=None if a.cpu else "cuda:0", **cap)
    if pool:
        relations, info = video.suppress(relations, a.rel_nms, video.MAX_PER_VIDEO, pool, device=None if a.cpu else "cuda:0")
        print(video.nms_totals(info) + " (vIoU %g)" % a.rel_nms)
    if a.associate == "tracks":
        mode = " along tracks (max_gap %d, %d gap frames bridged)" % (a.max_gap, video.gap_frames(relations))
    out = os.path.join(out_dir, "video_relations.json")
    with open(out, "w") as f:
        json.dump(relations, f)
    print("association%s: %d videos, %d relations, %.1f ms; wrote %s" % (
        mode, len(relations), sum(len(r) for r in relations.values()), 1e3 * (time.time() - t0), out))
    if a.save_videofeat_path:
        t0 = time.time()
        pooled = rf.pool(relations, sink.arena, device=None if a.cpu else "cuda:0")
        dt = time.time() - t0
        written, _ = rf.write(pooled, relations, a.save_videofeat_path)
        print(rf.report(relations, pooled, dt) + "; wrote %d files under %s" % (written, a.save_videofeat_path))
    return relations


if __name__ == "__main__":
    main()
