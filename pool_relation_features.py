#!/usr/bin/env python3
"""Video relation features from files, the reference's two-step flow (lib/utils.py:100-132 generate_static_relation_feat): the
relations of ``video_relations.json`` (``video_sgg_emb.py``) and the per-frame features ``<frame_feats>/<vid>/<fno>.npz``
(``pre_feat``; ``video_sgg_emb.py --save_feat_path DIR --save_frame_feats``) give ``<save_videofeat_path>/<predicate>/<vid>_<pno>.npy``,
one pooled feature per relation.  The rules are ``i2vsgg_amd.relation_features``'; ``--cpu`` pools on the host (no GPU needed),
otherwise the rows are uploaded once and pooled in one kernel launch.  A relation none of whose frames has a file gets no file
(the reference writes NaN there); their number is printed."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main(argv=None):
    p = argparse.ArgumentParser(description="Pool per-frame pair features into one feature per video relation")
    p.add_argument("--relations", required=True, help="video_relations.json")
    p.add_argument("--frame_feats", required=True, help="directory of <vid>/<fno>.npz files (pre_feat)")
    p.add_argument("--save_videofeat_path", required=True)
    p.add_argument("--cpu", action="store_true", help="host implementation of the pooling")
    a = p.parse_args(argv)
    from i2vsgg_amd import relation_features as rf
    with open(a.relations) as f:
        relations = json.load(f)
    store = rf.from_files(a.frame_feats)
    t0 = time.time()
    pooled = rf.pool(relations, store, device=None if a.cpu else "cuda:0")
    dt = time.time() - t0
    written, _ = rf.write(pooled, relations, a.save_videofeat_path)
    print(rf.report(relations, pooled, dt) + "; wrote %d files under %s" % (written, a.save_videofeat_path))
    return pooled


if __name__ == "__main__":
    main()
