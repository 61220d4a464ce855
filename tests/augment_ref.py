"""Float64 restatement of one view of grip_amd.augment for ONE plane: crop the box, resample it to n x n with Pillow's antialiased bicubic
(precompute_coeffs applied to the box, a = -0.5), mirror left-right when asked.  Returns, per output element, the reference value, the magnitude
A = sum |w_v| |w_h| |x| its rounding errors scale with, and the tap counts of its row and column.  Nothing here touches the product."""
import math

import numpy as np


def _bicubic(x, a=-0.5):
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def axis_weights(in_size, out_size):
    """(dense float64 weights [out, in], tap counts [out]) of Pillow's precompute_coeffs for in_size -> out_size."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    dense = np.zeros((out_size, in_size), dtype=np.float64)
    counts = np.zeros(out_size, dtype=np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - xmin
        w = _bicubic((np.arange(count, dtype=np.float64) + xmin - center + 0.5) * (1.0 / fs))
        s = math.fsum(w)
        if s != 0.0:
            w = w / s
        dense[xx, xmin:xmin + count] = w
        counts[xx] = count
    return dense, counts


def view_plane(plane, box, n, flip=False):
    """plane [H, W] (any float dtype), box = (top, left, height, width) -> (ref, A, T_v, T_h), each float64 / int64 [n, n]."""
    top, left, h, w = (int(v) for v in box[:4])
    crop = np.asarray(plane, dtype=np.float64)[top:top + h, left:left + w]
    wv, tv = axis_weights(h, n)
    wh, th = axis_weights(w, n)
    ref = wv @ crop @ wh.T
    A = np.abs(wv) @ np.abs(crop) @ np.abs(wh).T
    T_v = np.repeat(tv[:, None], n, axis=1)
    T_h = np.repeat(th[None, :], n, axis=0)
    if flip:
        ref, A, T_h = ref[:, ::-1], A[:, ::-1], T_h[:, ::-1]
    return np.ascontiguousarray(ref), np.ascontiguousarray(A), T_v, np.ascontiguousarray(T_h)
