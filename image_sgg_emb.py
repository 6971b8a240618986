#!/usr/bin/env python3
"""Relation test loop up to image-level recall@K: the per-frame part is ``test_sgg_emb.py``'s, unchanged (same flags, same
``relations.pkl``); its top-100 triplets per frame are then scored against ``--image_groundtruth``, a pickle of {frame: {boxes,
box_classes, rels}} (the layout of ``--target_gt_rels_path``), and relation / phrase detection recall@50/100 with zero-shot and
per-predicate recall is printed and written to ``image_relations.json`` beside ``relations.pkl`` (``eval_image_relations.py``, which
scores a written file the same way; the rules: i2vsgg_amd/image_relations.py).  On annotated boxes relation-mode recall IS
predicate-detection recall; with ``--target_gt_rels_path tracked_boxes.pkl`` it is relation detection.  ``--train_annotations``
defines the seen triplets of the zero-shot split.  Every other argument goes to ``test_sgg_emb.py``."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


def main(argv=None):
    p = argparse.ArgumentParser(description="Relation test loop + image relation recall@K on MI355X", add_help=False)
    p.add_argument("--image_groundtruth", required=True)
    p.add_argument("--train_annotations", default="")
    p.add_argument("--k_per_pair", type=int, default=None)
    p.add_argument("--nreturns", type=int, nargs="+", default=[50, 100])
    p.add_argument("--iou", type=float, default=0.5)
    p.add_argument("--cpu", action="store_true", help="host implementation of the match and the counters")
    a, rest = p.parse_known_args(argv)
    import eval_image_relations
    import test_sgg_emb as frames
    b = frames.parse_args(rest)
    results = frames.main(rest)
    out_dir = os.path.join(b.output_dir, b.net, b.dataset)
    extra = ["--nreturns"] + [str(k) for k in a.nreturns] + ["--iou", repr(a.iou)]
    extra += ["--train_annotations", a.train_annotations] if a.train_annotations else []
    extra += ["--k_per_pair", str(a.k_per_pair)] if a.k_per_pair is not None else []
    extra += ["--cpu"] if a.cpu else []
    metrics = eval_image_relations.main(["--prediction", os.path.join(out_dir, "relations.pkl"), "--groundtruth", a.image_groundtruth,
                                         "--num_relations", str(b.num_relations), "--out", os.path.join(out_dir, "image_relations.json")] + extra)
    return results, metrics


if __name__ == "__main__":
    main()
