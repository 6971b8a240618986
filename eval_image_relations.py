#!/usr/bin/env python3
"""Score the relation test loop's triplets against image-level annotations after the fact: relation detection and phrase
detection recall@K of image relation work (Lu et al., ECCV 2016), zero-shot recall and per-predicate ("mean") recall.
``--prediction`` is the ``relations.pkl`` that ``test_sgg_emb.py`` writes ({frame: (rlp_labels, tuple_confs, sub_bboxes,
obj_bboxes, rel_idex)}); ``--groundtruth`` a pickle of {frame: {boxes, box_classes, rels}} (the layout of
``--target_gt_rels_path``).  Frames are matched by key; a prediction key that is a path is also tried by its file name.  On
annotated boxes relation-mode recall IS predicate-detection recall.  ``--train_annotations`` (same layout) defines the seen
triplets of the zero-shot split; ``--k_per_pair`` caps the written list per pair of boxes.  The match and the counters run on
the GPU; ``--cpu`` runs the same rules on the host.  The rules: i2vsgg_amd/image_relations.py."""
import argparse
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


def by_annotation_key(relations, annotations):
    """The loop keys its results by image path and the annotation dicts by file name: a key that is not annotated is renamed to
    its file name where that one is (and no other prediction already has that name)."""
    out = {}
    for key, rec in relations.items():
        name = key.split("/")[-1] if isinstance(key, str) else key
        out[name if key not in annotations and name in annotations and name not in relations else key] = rec
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description="Image relation recall@K of per-frame triplets")
    p.add_argument("--prediction", required=True)
    p.add_argument("--groundtruth", required=True)
    p.add_argument("--num_relations", type=int, required=True)
    p.add_argument("--train_annotations", default="", help="annotations of the training set: their triplets are the seen ones")
    p.add_argument("--k_per_pair", type=int, default=None, help="keep at most k rows per pair of boxes of the written list")
    p.add_argument("--nreturns", type=int, nargs="+", default=[50, 100])
    p.add_argument("--iou", type=float, default=0.5)
    p.add_argument("--cpu", action="store_true", help="host implementation (no GPU needed)")
    p.add_argument("--out", default="image_relations.json")
    a = p.parse_args(argv)
    from i2vsgg_amd import image_relations
    with open(a.prediction, "rb") as f:
        prediction = pickle.load(f)
    with open(a.groundtruth, "rb") as f:
        groundtruth = pickle.load(f, encoding="bytes")
    seen = None
    if a.train_annotations:
        with open(a.train_annotations, "rb") as f:
            seen = image_relations.seen_triplets_of(pickle.load(f, encoding="bytes"))
    print("Number of images in ground truth: %d" % len(groundtruth))
    print("Number of images in prediction: %d" % len(prediction))
    res = image_relations.evaluate(by_annotation_key(prediction, groundtruth), groundtruth, a.num_relations, tuple(a.nreturns), a.iou,
                                   a.k_per_pair, seen, device=None if a.cpu else "cuda:0")
    image_relations.report(res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(image_relations.to_json(res), f, indent=1)
        print("wrote %s" % a.out)
    return res


if __name__ == "__main__":
    main()
