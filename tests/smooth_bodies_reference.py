"""Ground truth of the smooth splat of rigid bodies (include/dpr.h, SMOOTH SPLAT, RIGID BODIES): the numpy smooth
reference (tests/smooth_reference.py) composed per body, exactly as tests/bodies_reference.py composes the oracle.

With background 0, plane b of `raster_smooth_bodies` is the sum over k of raster_smooth of the points with body == k
under pose (b, k); every gradient is the matching piece of raster_pullback_smooth of that subset, and ds_dout_weight
adds over k.  Points whose body lies outside [0, K) belong to no subset: they deposit nothing and keep zero
gradients.  No arithmetic here beyond those sums, in the dtype asked for."""
import numpy as np

from tests import smooth_reference as SR


def _subsets(body, K):
    body = np.asarray(body)
    for k in range(K):
        idx = np.flatnonzero(body == k)
        if idx.size:
            yield k, idx


def _pw(point_weight, idx):
    return None if point_weight is None else np.asarray(point_weight)[idx]


def raster(grid_size, points, body, rotation, translation, background=None, out_weight=None, point_weight=None,
           dtype=np.float64):
    """points (P, n_in), body (P,), rotation (B, K, n_out, n_in), translation (B, K, n_out) -> grid_size + (B,)"""
    rotation, translation = np.asarray(rotation), np.asarray(translation)
    B, K = rotation.shape[:2]
    out = np.zeros(tuple(grid_size) + (B,), dtype=dtype)
    for k, idx in _subsets(body, K):
        out += SR.raster_smooth(grid_size, np.asarray(points)[idx], rotation[:, k], translation[:, k], None,
                                out_weight, _pw(point_weight, idx), dtype=dtype)
    if background is not None:
        out += np.asarray(background, dtype=dtype)
    return out


def raster_pullback(ds_dout, points, body, rotation, translation, out_weight=None, point_weight=None,
                    dtype=np.float64):
    """-> (ds_dpoints (P, n_in), ds_drotation (B, K, n_out, n_in), ds_dtranslation (B, K, n_out), ds_dbackground (B,),
    ds_dout_weight (B,), ds_dpoint_weight (P,))"""
    rotation, translation, points = np.asarray(rotation), np.asarray(translation), np.asarray(points)
    B, K, n_out, n_in = rotation.shape
    P = points.shape[0]
    d_pts, d_pw = np.zeros((P, n_in), dtype=dtype), np.zeros((P,), dtype=dtype)
    d_rot, d_trans = np.zeros((B, K, n_out, n_in), dtype=dtype), np.zeros((B, K, n_out), dtype=dtype)
    d_ow = np.zeros((B,), dtype=dtype)
    # (the grid sum: the same from every subset, and from none)
    d_bg = SR.raster_pullback_smooth(ds_dout, points[:0], rotation[:, 0], translation[:, 0], out_weight, None,
                                     dtype=dtype)[3]
    for k, idx in _subsets(body, K):
        r = SR.raster_pullback_smooth(ds_dout, points[idx], rotation[:, k], translation[:, k], out_weight,
                                      _pw(point_weight, idx), dtype=dtype)
        d_pts[idx], d_pw[idx] = r[0], r[5]
        d_rot[:, k], d_trans[:, k] = r[1], r[2]
        d_ow += r[4]
    return d_pts, d_rot, d_trans, d_bg, d_ow, d_pw
