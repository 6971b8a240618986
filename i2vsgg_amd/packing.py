"""What the host packers of the packed-table ops share (seqnms, relation_targets, image_relations, detection_eval, video):
the +1 overlap that three of them match boxes with, and the two steps every ``pack`` ends in.  numpy only: the host modules
stay importable without the library.
"""
import numpy as np


def overlap_plus1(a, b):
    """(n, 4) against (m, 4) float64 boxes -> (n, m) overlaps, the rule the kernels keep bit for bit
    (csrc/table_common.h, ``i2v_overlap_plus1``).  The +1 convention of lib/model/nms/nms_cpu.py:14,26-31 in this operation
    order: ``iw = (min(x2) - max(x1)) + 1``, ``ih`` likewise; 0 if either is ``<= 0``, else ``iw*ih / ((area_a + area_b) -
    iw*ih)`` with ``area = ((x2 - x1) + 1) * ((y2 - y1) + 1)``."""
    iw = (np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])) + 1.0
    ih = (np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])) + 1.0
    inter = iw * ih
    aa = ((a[:, 2] - a[:, 0]) + 1.0) * ((a[:, 3] - a[:, 1]) + 1.0)
    ab = ((b[:, 2] - b[:, 0]) + 1.0) * ((b[:, 3] - b[:, 1]) + 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ov = inter / ((aa[:, None] + ab[None, :]) - inter)
    return np.where((iw <= 0.0) | (ih <= 0.0), 0.0, ov)


def offsets(counts, what):
    """Row counts (n) -> the int32 offset table (n + 1).  The kernels index with int32: a total of 2^31 or more is a
    ``ValueError`` with the message ``what``."""
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts, np.int64), out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError(what)
    return off.astype(np.int32)


def cat(parts, tail_shape, dtype):
    """A list of arrays -> one C-contiguous ``dtype`` array of shape (-1,) + tail_shape; an empty list gives zero rows."""
    if not parts:
        return np.zeros((0,) + tuple(tail_shape), dtype)
    return np.ascontiguousarray(np.concatenate(parts).astype(dtype).reshape((-1,) + tuple(tail_shape)))
