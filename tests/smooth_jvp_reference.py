"""numpy restatement of the forward-mode derivative of the smooth splat (include/dpr.h, SMOOTH SPLAT, FORWARD MODE),
on the per-pose terms of tests/smooth_reference.py: any dtype, batched, K leading.  The CPU reference of
tests/test_smooth_jvp_reference.py and tests/test_smooth_jvp_gpu.py.

Shapes: the primals as in tests/smooth_reference.py; tangents (None = zero) points_dot (K, P, N_in), rotation_dot
(K, B, N_out, N_in), translation_dot (K, B, N_out), background_dot / out_weight_dot (K, B), point_weight_dot (K, P).
Returns out_dot of shape grid + (K, B).
"""
import itertools

import numpy as np

from tests.smooth_reference import _defaults, _terms


def raster_smooth_jvp(grid, points, rotation, translation, out_weight=None, point_weight=None, *, K,
                      points_dot=None, rotation_dot=None, translation_dot=None, background_dot=None,
                      out_weight_dot=None, point_weight_dot=None, dtype=np.float64, magnitudes=False):
    """out_dot.  With `magnitudes` the same deposit loop on |v|: (A, n) with A of shape grid + (K, B), the sum of the
    absolute values of the deposits on a cell plus |background_dot|, and n of shape grid + (B,), their number."""
    dtype = np.dtype(dtype).type
    grid = tuple(int(g) for g in grid)
    N, B, P = len(grid), rotation.shape[0], points.shape[0]
    n_in = points.shape[1]
    _bg, ow, pw = _defaults(B, P, None, out_weight, point_weight, dtype)
    pts = np.asarray(points, dtype=dtype)
    n = np.asarray(grid, dtype=dtype)

    def tan(t, shape):
        return np.zeros(shape, dtype) if t is None else np.asarray(t, dtype=dtype).reshape(shape)

    pd, Rd = tan(points_dot, (K, P, n_in)), tan(rotation_dot, (K, B, N, n_in))
    td, bgd = tan(translation_dot, (K, B, N)), tan(background_dot, (K, B))
    owd, pwd = tan(out_weight_dot, (K, B)), tan(point_weight_dot, (K, P))
    out = np.empty(grid + (K, B), dtype=dtype)
    count = np.zeros(grid + (B,), np.int64)
    for b, idx, j0, w, dw in _terms(grid, points, rotation, translation, dtype):
        R = np.asarray(rotation[b], dtype=dtype)
        # (K, A, ..): a rejected point's tangents are never read (idx holds the accepted points only)
        cdot = (pts[idx] @ np.swapaxes(Rd[:, b], 1, 2) + pd[:, idx] @ R.T + td[:, b, None, :]) * (n / dtype(2))
        a = owd[:, b, None] * pw[idx] + ow[b] * pwd[:, idx]
        c = ow[b] * pw[idx]
        planes = np.empty((K,) + grid, dtype=dtype)
        planes[...] = bgd[:, b].reshape((K,) + (1,) * N)
        if magnitudes:
            planes = np.abs(planes)
        hits = np.zeros(grid, np.int64)
        for s in itertools.product(range(3), repeat=N):
            cell = j0 + (np.asarray(s) - 1)
            inside = np.all((cell >= 0) & (cell < np.asarray(grid)), axis=1)
            v = a.copy()
            for d in range(N):
                v = v * w[:, d, s[d]]
            for m in range(N):
                term = c * cdot[:, :, m] * dw[:, m, s[m]]
                for d in range(N):
                    if d != m:
                        term = term * w[:, d, s[d]]
                v = v + term
            if magnitudes:
                v = np.abs(v)
            np.add.at(planes, (slice(None),) + tuple(cell[inside].T), v[:, inside])
            np.add.at(hits, tuple(cell[inside].T), 1)
        out[..., b] = np.moveaxis(planes, 0, -1)
        count[..., b] = hits
    return (out, count) if magnitudes else out
