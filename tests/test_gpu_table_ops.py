"""The packed-table ops' binding module (i2vsgg_amd/table_ops.py): ``ops`` re-exports the same functions, a device that is
not a GPU is refused under the name of the op's host form, and a batch without entries comes back as empty outputs of the
documented dtypes.  What the kernels compute is the matter of the per-op test files; nothing here launches more than an
empty call."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_i = lambda *v: np.asarray(v, np.int32)
_z = lambda *shape: np.zeros(shape, np.float64)
I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64

# op -> (the host form its refusal names, one well-formed entry, a batch without entries, the (shape, dtype) of every output)
CASES = {
    "video_associate": ("video.associate(device=None)",
                        (_i(0, 1), _i(0), _i(0, 1), [0.5], _i(1, 2, 3).reshape(1, 3), _z(1, 8)),
                        (_i(0), _i(), _i(0), _z(0), np.zeros((0, 3), np.int32), _z(0, 8)),
                        [((0,), I32), ((0,), I32), ((0,), I32), ((0,), F64), ((0,), I32)]),
    "video_viou_match": ("video.match(device=None)",
                         (_i(0, 1), np.zeros((1, 10), np.int32), [0.5], _i(0, 1), np.zeros((1, 10), np.int32), _z(1, 4)),
                         (_i(0), np.zeros((0, 10), np.int32), _z(0), _i(0), np.zeros((0, 10), np.int32), _z(0, 4)),
                         [((0, 0), F64), ((0,), I32), ((0,), F64)]),
    "seq_nms": ("seqnms.seq_nms(device=None)",
                (_i(0, 1), _i(0), _i(0, 1), np.zeros((1, 4), np.float32), np.zeros(1, np.float32)),
                (_i(0), _i(), _i(0), np.zeros((0, 4), np.float32), np.zeros(0, np.float32)),
                [((0,), I32), ((0,), F32), ((0,), I32)]),
    "relation_targets": ("relation_targets.relation_targets_host",
                         (_i(0, 1), _z(1, 4), _i(1), _i(0, 1), _z(1, 4), _i(1), _i(0, 1), _i(0, 0, 0).reshape(1, 3),
                          np.zeros((1, 10), np.uint32), [100.0], [100.0], 3),
                         (_i(0), _z(0, 4), _i(), _i(0), _z(0, 4), _i(), _i(0), np.zeros((0, 3), np.int32),
                          np.zeros((0, 10), np.uint32), _z(0), _z(0), 3),
                         {"rel5": ((0, 5), F32), "bounds": ((0, 2, 4), I32), "labels": ((0, 3), F32), "ixs": ((0,), I64),
                          "ixo": ((0,), I64), "w": ((0,), F32), "n_pairs": ((0,), I32), "n_dropped": ((0,), I32),
                          "samp": ((0, 10, 2), I32), "status": ((), I32)}),
    "recognition_rows": ("eval.recognition_rows_host",
                         (np.ones((1, 2), np.float32), np.ones((1, 1), np.float32), [0], [0], _z(1, 1, 1)),
                         (np.ones((0, 2), np.float32), np.ones((0, 1), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64),
                          _z(1, 1, 1)),
                         [((0, 2), F32), ((0, 2), F32), ((0, 1), F32), ((0,), I32)]),
    "recognition_align": ("recognition.align_arrays_host",
                          (_z(1, 5), _i(0, 1), _i(0), _i(0, 1, 0, 1).reshape(1, 4), 2, 1),
                          (_z(0, 5), _i(0), _i(), np.zeros((0, 4), np.int32), 2, 1),
                          [((0, 5), F64), ((0,), I32), ((0, 3, 10), I32), ((0, 7), I32), ((8,), I64), ((2, 2, 2), I64)]),
    "image_relation_match": ("image_relations.match_host",
                             (_i(0, 1), _i(0, 1), _i(1, 2, 3).reshape(1, 3), _z(1, 8), _i(1, 2, 3).reshape(1, 3), _z(1, 8)),
                             (_i(0), _i(0), np.zeros((0, 3), np.int32), _z(0, 8), np.zeros((0, 3), np.int32), _z(0, 8)),
                             [((2, 0), I32), ((2, 0), F64), ((2, 0), I32)]),
    "image_relation_count": ("image_relations.count_host",
                             (np.zeros((2, 1), np.int32), _i(1, 2, 3).reshape(1, 3), _i(0), (50,), 5),
                             (np.zeros((2, 0), np.int32), np.zeros((0, 3), np.int32), _i(), (50,), 5),
                             [((2, 1, 2), I64), ((2, 1, 2), I64), ((2, 1, 5, 2), I64)]),
    "relation_feature_pool": ("relation_features.pool_arrays_host",
                              (np.ones((1, 4), np.float32), _i(0, 1), _i(0, 1), _i(0), _i(0)),
                              (np.ones((0, 4), np.float32), _i(0), _i(0), _i(), _i()),
                              [((0, 4), F32), ((0,), I32)]),
    "det_eval_match": ("detection_eval.match_arrays_host",
                       (_i(0, 1), _i(0), _i(0, 1), _i(5), _z(1, 4), _z(1, 4), _i(0)),
                       (_i(0), _i(), _i(0), _i(), _z(0, 4), _z(0, 4), _i()),
                       [((0,), I32), ((0,), F64), ((0,), I32)]),
    "det_eval_curve": ("detection_eval.curve_arrays_host",
                       (_i(5), _i(0, 1), _i(1), _i(1)),
                       (_i(), _i(0), _i(), _i()),
                       [((0,), I32), ((0,), I32), ((0,), I32), ((0,), F64), ((0,), F64), ((0,), F64), ((0,), F64)]),
}
# tensors only: rel_score (n_pairs, n_rel), conf (n_boxes), ixs, ixo (n_pairs)
_topk = lambda n, dev: (torch.ones((n, 2), device=dev), torch.ones((2,), device=dev), torch.zeros((n,), dtype=I64, device=dev),
                        torch.ones((n,), dtype=I64, device=dev))
OPS = ["relation_topk"] + list(CASES)


@pytest.mark.parametrize("name", OPS)
def test_table_op_is_reexported_refuses_the_cpu_and_takes_an_empty_batch(name):
    from i2vsgg_amd import _lib, ops, table_ops
    op = getattr(table_ops, name)
    assert getattr(ops, name) is op
    if name == "relation_topk":
        with pytest.raises(_lib.I2VError, match="no CPU fallback"):
            op(*_topk(1, "cpu"))
        got, want = op(*_topk(0, DEV)), [((0,), I32), ((0,), I32), ((0,), F32)]
    else:
        host_form, one, none, want = CASES[name]
        with pytest.raises(_lib.I2VError) as e:
            op(*one, device="cpu")
        assert "run on the GPU only" in str(e.value) and ("%s is the host form" % host_form) in str(e.value)
        got = op(*none, device=DEV)
    if isinstance(want, dict):
        assert set(got) == set(want)
        got, want = [got[k] for k in want], list(want.values())
    assert len(got) == len(want)
    for t, (shape, dtype) in zip(got, want):
        assert t.device == torch.device(DEV) and tuple(t.shape) == shape and t.dtype == dtype, (name, t.shape, t.dtype, shape, dtype)
        assert not t.any()                                       # the counters of an empty batch are zero, its status word 0
