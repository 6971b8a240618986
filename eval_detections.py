#!/usr/bin/env python3
"""Score pickled detections against an imdb's annotations (the ``imdb.evaluate_detections`` call that ends
test_net_instance_styleD.py): VOC AP per class and the mean AP.  ``--detections`` is the ``detections.pkl`` that
``test_instance_styled.py`` writes, ``all_boxes[class][image]``; ``--imdbval_name`` names the imdb it was run on.  The match
and the curves run on the GPU; ``--cpu`` runs the same rules on the host."""
import argparse
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


def main(argv=None):
    p = argparse.ArgumentParser(description="VOC detection AP of pickled detections")
    p.add_argument("--detections", required=True)
    p.add_argument("--imdbval_name", required=True)
    p.add_argument("--ovthresh", type=float, default=0.5)
    p.add_argument("--voc07", action="store_true", help="the 11-point AP of the 2007 devkit")
    p.add_argument("--cpu", action="store_true", help="host implementation (no GPU needed)")
    p.add_argument("--output_dir", default=None, help="also write <cls>_pr.pkl and detection_eval.json there")
    a = p.parse_args(argv)
    from i2vsgg_amd import detection_eval
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    with open(a.detections, "rb") as f:
        all_boxes = pickle.load(f)
    imdb = get_imdb(a.imdbval_name)
    n = len(all_boxes[0]) if len(all_boxes) else 0
    print("%d classes, %d images" % (len(imdb.classes) - 1, n))
    res = detection_eval.evaluate(all_boxes, imdb.roidb[:n], imdb.classes, a.ovthresh, a.voc07, device=None if a.cpu else "cuda:0")
    if a.output_dir:
        os.makedirs(a.output_dir, exist_ok=True)
    print("VOC07 metric? " + ("Yes" if a.voc07 else "No"))
    detection_eval.report(res, imdb.classes, a.output_dir)
    return res


if __name__ == "__main__":
    main()
