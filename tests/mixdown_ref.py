"""numpy restatement of asx_mixdown_batch_dev (csrc/kernels_mix.h): one job.

    acc = fl(w_0 * x_0);  acc = fl(acc + fl(w_k * x_k)), k = 1 .. K-1 in list order

float32, one rounding per operation (numpy multiplies and adds element by element, without contraction), a source shorter than
``n_out`` read as zeros behind its end, one longer read up to ``n_out``.  ``mixdown_exact`` is the same sum in float64 together with
``sum |w_k x_k|``, the quantity the rounding-error bound of a recursive float32 sum is stated against."""
from __future__ import annotations

import numpy as np


def _planar(a, layout, n_out, dtype):
    a = np.asarray(a, np.float32)
    a = a if layout == "planar" else a.T
    assert a.ndim == 2 and a.shape[0] == 2, a.shape
    x = np.zeros((2, n_out), dtype)
    m = min(n_out, a.shape[1])
    x[:, :m] = a[:, :m]
    return x


def mixdown_ref(sources, n_out, out_layout="planar"):
    """``sources``: [(float32 array [2, n] or [n, 2], "planar" | "rows", weight)] -> float32 [2, n_out] or [n_out, 2]."""
    acc = None
    for a, layout, w in sources:
        term = np.multiply(np.float32(w), _planar(a, layout, n_out, np.float32), dtype=np.float32)
        acc = term if acc is None else np.add(acc, term, dtype=np.float32)
    return np.ascontiguousarray(acc if out_layout == "planar" else acc.T)


def mixdown_exact(sources, n_out):
    """(sum_k w_k x_k, sum_k |w_k x_k|) in float64, planar [2, n_out]; the weights are the float32 values the kernel is given."""
    total, mass = np.zeros((2, n_out)), np.zeros((2, n_out))
    for a, layout, w in sources:
        term = np.float64(np.float32(w)) * _planar(a, layout, n_out, np.float64)
        total += term
        mass += np.abs(term)
    return total, mass
