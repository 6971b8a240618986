#!/usr/bin/env python3
"""Score per-frame recognitions against video-level annotations after the fact (the ``alignment`` / ``evaluate_recognition``
calls that end the ``pre_det`` branch of test_net_SGG_emb.py, :318-324): subject, object and predicate accuracy@1 / @5,
relationship accuracy@1 and per-class object accuracy.  ``--prediction`` is the ``frame_recognitions.pkl`` that
``recognize_sgg_emb.py`` writes; ``--groundtruth`` a JSON of VidVRD-style relations ({video: [{triplet, subject_tid, object_tid,
duration}]}), or the ``recognition.json`` of a run, which carries its ground truth and names.  The alignment and the counting
run on the GPU; ``--cpu`` runs the same rules on the host."""
import argparse
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


def main(argv=None):
    p = argparse.ArgumentParser(description="Predicate recognition accuracy of per-frame scores")
    p.add_argument("--prediction", required=True)
    p.add_argument("--groundtruth", required=True)
    p.add_argument("--classes", default="", help="JSON list of class names, background first (default: the ground truth "
                   "file's own, else class1, class2, ...; integer labels need no names)")
    p.add_argument("--predicates", default="", help="JSON list of predicate names or {name: label}")
    p.add_argument("--cpu", action="store_true", help="host implementation (no GPU needed)")
    a = p.parse_args(argv)
    from i2vsgg_amd import recognition
    with open(a.prediction, "rb") as f:
        prediction = pickle.load(f)
    with open(a.groundtruth) as f:
        groundtruth = json.load(f)
    classes = predicates = None
    if "groundtruth" in groundtruth and "metrics" in groundtruth:            # a run's recognition.json
        classes, predicates, groundtruth = groundtruth["classes"], groundtruth["predicates"], groundtruth["groundtruth"]
    if a.classes:
        with open(a.classes) as f:
            classes = json.load(f)
    n_classes, n_rel = recognition.widths(prediction)       # the score rows say how many classes and predicates there are
    if classes is None:
        classes = ["__background__"] + ["class%d" % i for i in range(1, n_classes)]
    if a.predicates or predicates is None:
        predicates = recognition.predicate_names(a.predicates, n_rel)
    print("Number of videos in ground truth: %d" % len(groundtruth))
    print("Number of videos in prediction: %d" % len(prediction))
    res = recognition.evaluate(prediction, groundtruth, classes, predicates, device=None if a.cpu else "cuda:0")
    recognition.report(res, classes)
    return res


if __name__ == "__main__":
    main()
