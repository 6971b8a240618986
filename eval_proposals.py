#!/usr/bin/env python3
"""Proposal / detection recall of pickled candidate boxes against an imdb's annotations: recall at IoU 0.5 ... 0.95 and the
average recall per candidate budget and object size (i2vsgg_amd/proposal_eval.py has the rules).  ``--candidates`` is the
``proposals.pkl`` that ``proposals_instance_styled.py`` writes (one (n, 4) array per image, best first) or a
``detections.pkl`` (``all_boxes[class][image]``: an image's candidates are its detections of all foreground classes in class
order, sorted by score descending, a stable sort); ``--imdbval_name`` names the imdb it was run on.  The cover runs on the
GPU; ``--cpu`` runs the same rules on the host."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")     # before HIP initialises: i2vsgg_amd/__init__.py


def _limit(text):
    return None if text == "all" else int(text)


def main(argv=None):
    from i2vsgg_amd import proposal_eval
    p = argparse.ArgumentParser(description="Recall and average recall of pickled proposals or detections")
    p.add_argument("--candidates", required=True, help="proposals.pkl or detections.pkl")
    p.add_argument("--imdbval_name", required=True)
    p.add_argument("--limits", nargs="+", type=_limit, default=list(proposal_eval.DEFAULT_LIMITS), help="candidate budgets; 'all': no limit")
    p.add_argument("--areas", nargs="+", default=list(proposal_eval.DEFAULT_AREAS), choices=list(proposal_eval.AREAS))
    p.add_argument("--cpu", action="store_true", help="host implementation (no GPU needed)")
    p.add_argument("--out", default=None, help="also write the result there as JSON (proposal_recall.json)")
    a = p.parse_args(argv)
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    cands = proposal_eval.load_candidates(a.candidates)
    imdb = get_imdb(a.imdbval_name)
    n = len(cands)
    if n != len(imdb.roidb):                              # a partial file would score a subset without saying so
        raise SystemExit("eval_proposals: %s holds %d images, %s has %d" % (a.candidates, n, a.imdbval_name, len(imdb.roidb)))
    print("%d images, %d candidates" % (n, sum(len(c) for c in cands)))
    res = proposal_eval.evaluate(cands, imdb.roidb, a.limits, a.areas, device=None if a.cpu else "cuda:0",
                                 num_classes=imdb.num_classes)
    proposal_eval.report(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(proposal_eval.to_json(res), f, indent=1)
    return res


if __name__ == "__main__":
    main()
