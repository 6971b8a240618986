"""Seeded inputs of the video-relation-feature tests (host and GPU) and the plain reference they are held to.

A case is the kernel's own arrays: ``feat`` (n_rows, dim) float32, ``slot_off``, ``mem_off``, ``mem_slot``, ``mem_idx``.  The values
mix magnitudes (about 1e-3 to 1e6) and both signs, so that a float32 sum depends on its order: ``assert_order_sensitive`` proves
it for every case it is given, on the CPU -- without that the "member order" tests would prove nothing."""
import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_relation_feat.npz")
BATCH = 4                    # csrc/relation_features.hip RF_BATCH: rows whose loads are in flight together
PASS_WIDE = 512              # columns of one pass with 16-byte loads (2 groups x 64 lanes x 4), 128 with 4-byte loads
PASS_NARROW = 128


def values(rng, shape):
    """float32 of both signs, magnitudes log-uniform over 1e-3 .. 1e6."""
    mag = 10.0 ** rng.uniform(-3.0, 6.0, size=shape)
    return (mag * rng.choice([-1.0, 1.0], size=shape)).astype(F32)


def sequential_mean(rows):
    """The rule, spelled out: float32 adds in the given order starting FROM the first row, then one float32 division."""
    rows = np.asarray(rows, F32)
    acc = rows[0].copy()
    for row in rows[1:]:
        acc = (acc + row).astype(F32)
    return (acc / F32(len(rows))).astype(F32)


def make_case(seed, dim, counts, n_slots=9, max_pairs=6, skip="none"):
    """One relation per entry of ``counts`` (its number of members).  ``skip``: "none"; "some" (about a third of the members
    have no slot); "first" (the first two members of every relation have none: the sum must start from the first VALID row);
    "all" (no member has a slot: count 0, zeros)."""
    rng = np.random.default_rng(seed)
    n_pairs = rng.integers(1, max_pairs + 1, size=n_slots)
    slot_off = np.zeros(n_slots + 1, np.int32)
    np.cumsum(n_pairs, out=slot_off[1:])
    feat = values(rng, (int(slot_off[-1]), dim))
    mem_off = np.zeros(len(counts) + 1, np.int32)
    np.cumsum(np.asarray(counts, np.int64), out=mem_off[1:])
    M = int(mem_off[-1])
    mem_slot = rng.integers(0, n_slots, size=M).astype(np.int32)
    mem_idx = (rng.integers(0, 1 << 30, size=M) % n_pairs[mem_slot]).astype(np.int32)
    if skip == "some":
        mem_slot[rng.random(M) < 0.34] = -1
    elif skip == "all":
        mem_slot[:] = -1
    elif skip == "first":
        for r in range(len(counts)):
            mem_slot[mem_off[r]:min(mem_off[r] + 2, mem_off[r + 1])] = -1
    return {"feat": feat, "slot_off": slot_off, "mem_off": mem_off, "mem_slot": mem_slot, "mem_idx": mem_idx, "dim": dim}


def rows_of(case, r):
    """Row numbers of relation r's valid members, in member order."""
    m0, m1 = int(case["mem_off"][r]), int(case["mem_off"][r + 1])
    s, k = case["mem_slot"][m0:m1], case["mem_idx"][m0:m1]
    return (case["slot_off"][s[s >= 0]].astype(np.int64) + k[s >= 0])


def expected(case):
    """(pooled, count) by the spelled-out rule, relation by relation."""
    R = len(case["mem_off"]) - 1
    pooled, count = np.zeros((R, case["dim"]), F32), np.zeros(R, np.int32)
    for r in range(R):
        rows = rows_of(case, r)
        count[r] = len(rows)
        if len(rows):
            pooled[r] = sequential_mean(case["feat"][rows])
    return pooled, count


def assert_order_sensitive(case):
    """Every relation with at least three distinct valid rows and at least 64 columns sums differently in reversed member order
    in at least one column (a column of three values often does not: the largest swallows the rest, so a few columns are not
    enough to demand it of EVERY relation); a narrower case must hold at least one such relation, and more than half of its
    relations must be such.  (Two rows commute: a + b == b + a.)"""
    R = len(case["mem_off"]) - 1
    seen = differ = 0
    for r in range(R):
        rows = rows_of(case, r)
        if len(rows) < 3 or len(set(rows.tolist())) < 3:
            continue
        seen += 1
        d = (sequential_mean(case["feat"][rows]) != sequential_mean(case["feat"][rows[::-1]])).any()
        differ += int(d)
        assert d or case["dim"] < 64, "relation %d of %d rows sums to the same bits in both orders" % (r, len(rows))
    assert seen == 0 or 2 * differ > seen, "only %d of %d relations of the case depend on the member order" % (differ, seen)
    return seen, differ


MEMBER_COUNTS = [1, 2, BATCH - 1, BATCH, BATCH + 1, 63, 64, 65, 300]


def kernel_cases():
    """{name: case} of the device-against-host test: every path of the kernel at the smallest size that takes it."""
    out = {}
    # dim 300: 16-byte loads, 75 groups (lanes 0..10 hold a second group); 8: two lanes; 6 and 1: the 4-byte path
    for dim in (300, 8, 6, 1):
        out["dim%d" % dim] = make_case(100 + dim, dim, MEMBER_COUNTS)
    out["dim%d_two_passes" % (PASS_WIDE + 4)] = make_case(7, PASS_WIDE + 4, [1, 5, 70])
    out["dim%d_two_passes" % (PASS_NARROW + 3)] = make_case(8, PASS_NARROW + 3, [1, 5, 70])
    out["one_relation"] = make_case(9, 300, [37])
    out["thousand_relations"] = make_case(10, 8, list(np.random.default_rng(10).integers(0, 40, size=1000)), n_slots=50)
    out["some_skipped"] = make_case(11, 300, MEMBER_COUNTS, skip="some")
    out["first_skipped"] = make_case(12, 8, MEMBER_COUNTS, skip="first")
    out["all_skipped"] = make_case(13, 8, [1, 5, 64, 130], skip="all")
    shared = make_case(14, 12, [40, 40, 40], n_slots=2, max_pairs=3)          # at most 6 rows: every relation reads them all
    out["shared_rows"] = shared
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the golden's inputs (tools/gen_golden.py --only video_relation_feat runs the reference's own function on them)
# ---------------------------------------------------------------------------------------------------------------------
def golden_inputs():
    """[{dim, slots: [(vid, fno, rows)] in LOADER order (not frame order), relations: {vid: [{triplet, duration, rel_idex}]}}]:
    3 videos of at most 40 frames at dim 8, and a small case at dim 300.  Some frames inside a duration have no file; every
    relation has at least one frame of its own (the reference writes NaN otherwise)."""
    cases = []
    for seed, dim, n_frames, n_rel, max_pairs in ((21, 8, (40, 23, 31), 6, 6), (22, 300, (7, 5, 6), 2, 2)):
        rng = np.random.default_rng(seed)
        slots, relations = [], {}
        for v, F in enumerate(n_frames):
            vid = "vid%d" % v
            own = rng.random(F) < 0.8
            own[int(rng.integers(1, F - 1))] = False                         # at least one frame without a file, not at an end
            pairs = rng.integers(1, max_pairs + 1, size=F)
            for f in range(F):
                if own[f]:
                    slots.append((vid, f, values(rng, (int(pairs[f]), dim))))
            rels = []
            missing = np.nonzero(~own)[0]
            for k in range(n_rel):
                if k == 0:                                                   # one relation spans a frame without a file
                    hole = int(missing[(missing > 0) & (missing < F - 1)][0])
                    f0, f1 = max(hole - 3, 0), min(hole + 4, F)
                else:
                    f0 = int(rng.integers(0, F - 3))
                    f1 = int(rng.integers(f0 + 3, F + 1))
                if not own[f0:f1].any():
                    continue
                rels.append({"triplet": ["c%d" % rng.integers(0, 5), "p%d" % rng.integers(0, 4), "c%d" % rng.integers(0, 5)],
                             "duration": [f0, f1], "rel_idex": [int(rng.integers(0, pairs[f])) for f in range(f0, f1)]})
            relations[vid] = rels
        order = rng.permutation(len(slots))                                  # the loader's order depends on the aspect ratios
        cases.append({"dim": dim, "slots": [slots[i] for i in order], "relations": relations})
    return cases


def _rf():
    from i2vsgg_amd import relation_features
    return relation_features


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def load_golden():
    """[(store, video_relations, {(vid, pno): expected row})] from the file's arrays alone."""
    out = []
    with np.load(GOLDEN) as z:
        for c in range(int(z["n_cases"])):
            g = dict((k[len("c%d_" % c):], z[k]) for k in z.files if k.startswith("c%d_" % c))
            vids = [str(v) for v in g["vids"]]
            store = _rf().HostStore(g["feat"].shape[1])
            for s in range(len(g["slot_vid"])):
                store.append((vids[g["slot_vid"][s]], int(g["slot_fno"][s])), g["feat"][g["slot_off"][s]:g["slot_off"][s + 1]])
            relations, want = dict((v, []) for v in vids), {}
            for r in range(len(g["rel_vid"])):
                vid = vids[g["rel_vid"][r]]
                assert len(relations[vid]) == int(g["rel_pno"][r])
                relations[vid].append({"triplet": ["s", str(g["rel_pred"][r]), "o"], "duration": g["rel_dur"][r].tolist(),
                                       "rel_idex": g["idex"][g["idex_off"][r]:g["idex_off"][r + 1]].tolist()})
                want[(vid, int(g["rel_pno"][r]))] = g["pooled"][r]
            out.append((store, relations, want))
    return out
