"""Ground truth of smooth sampling at the points of rigid bodies (include/dpr.h, SMOOTH SAMPLING, RIGID BODIES): the
numpy smooth-sampling reference (tests/sample_smooth_reference.py) composed per body, exactly as
tests/smooth_bodies_reference.py composes the splat.

Column b of `values` restricted to the points with body == k is sample_smooth of that subset under pose (b, k); every
gradient is the matching piece of sample_smooth_pullback of that subset, and ds_dimage adds over k.  Points whose body
lies outside [0, K) belong to no subset: they sample 0, deposit nothing and keep zero gradients.  No arithmetic here
beyond those sums, in the dtype asked for."""
import numpy as np

from tests import sample_smooth_reference as SS
from tests.smooth_bodies_reference import _subsets


def sample(image, points, body, rotation, translation, dtype=np.float64):
    """image grid + (B,), points (P, n_in), body (P,), rotation (B, K, n_out, n_in), translation (B, K, n_out)
    -> values (P, B)"""
    rotation, translation, points = np.asarray(rotation), np.asarray(translation), np.asarray(points)
    B, K = rotation.shape[:2]
    values = np.zeros((points.shape[0], B), dtype=dtype)
    for k, idx in _subsets(body, K):
        values[idx] = SS.sample_smooth(image, points[idx], rotation[:, k], translation[:, k], dtype=dtype)
    return values


def sample_pullback(ds_dvalues, image, points, body, rotation, translation, dtype=np.float64):
    """-> (ds_dimage grid + (B,), ds_dpoints (P, n_in), ds_drotation (B, K, n_out, n_in), ds_dtranslation
    (B, K, n_out))"""
    rotation, translation, points = np.asarray(rotation), np.asarray(translation), np.asarray(points)
    dv, image = np.asarray(ds_dvalues), np.asarray(image)
    B, K, n_out, n_in = rotation.shape
    d_img = np.zeros(image.shape, dtype=dtype)
    d_pts = np.zeros((points.shape[0], n_in), dtype=dtype)
    d_rot, d_trans = np.zeros((B, K, n_out, n_in), dtype=dtype), np.zeros((B, K, n_out), dtype=dtype)
    for k, idx in _subsets(body, K):
        r = SS.sample_smooth_pullback(dv[idx], image, points[idx], rotation[:, k], translation[:, k], dtype=dtype)
        d_img += r[0]
        d_pts[idx] = r[1]
        d_rot[:, k], d_trans[:, k] = r[2], r[3]
    return d_img, d_pts, d_rot, d_trans
