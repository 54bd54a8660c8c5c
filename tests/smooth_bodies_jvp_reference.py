"""Ground truth of the forward-mode derivative of the smooth splat of rigid bodies (include/dpr.h, SMOOTH SPLAT, RIGID
BODIES, FORWARD MODE): the numpy smooth JVP (tests/smooth_jvp_reference.py) composed per body exactly as
tests/smooth_bodies_reference.py composes the forward.

Subset k of the points runs under pose [:, k] with the point tangents [:, idx] and the pose tangents [:, :, k];
out_weight and its tangent are shared; the result is the sum over k plus background_dot.  Points whose body lies
outside [0, K) belong to no subset: none of their tangents is read.  No arithmetic here beyond those sums.

Shapes: the primals as in tests/smooth_bodies_reference.py; tangents (None = zero) points_dot (V, P, N_in),
rotation_dot (V, B, K, N_out, N_in), translation_dot (V, B, K, N_out), background_dot / out_weight_dot (V, B),
point_weight_dot (V, P).  Returns out_dot of shape grid + (V, B)."""
import numpy as np

from tests import smooth_jvp_reference as JR
from tests.smooth_bodies_reference import _pw, _subsets


def raster_smooth_bodies_jvp(grid, points, body, rotation, translation, out_weight=None, point_weight=None, *, V,
                             points_dot=None, rotation_dot=None, translation_dot=None, background_dot=None,
                             out_weight_dot=None, point_weight_dot=None, dtype=np.float64):
    rotation, translation, points = np.asarray(rotation), np.asarray(translation), np.asarray(points)
    B, K = rotation.shape[:2]
    out = np.zeros(tuple(int(g) for g in grid) + (V, B), dtype=dtype)
    for k, idx in _subsets(body, K):
        out += JR.raster_smooth_jvp(
            grid, points[idx], rotation[:, k], translation[:, k], out_weight, _pw(point_weight, idx), K=V,
            points_dot=None if points_dot is None else np.asarray(points_dot)[:, idx],
            rotation_dot=None if rotation_dot is None else np.asarray(rotation_dot)[:, :, k],
            translation_dot=None if translation_dot is None else np.asarray(translation_dot)[:, :, k],
            background_dot=None, out_weight_dot=out_weight_dot,
            point_weight_dot=None if point_weight_dot is None else np.asarray(point_weight_dot)[:, idx], dtype=dtype)
    if background_dot is not None:
        out += np.asarray(background_dot, dtype=dtype)
    return out
