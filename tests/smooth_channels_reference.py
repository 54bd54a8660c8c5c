"""numpy restatement of the smooth splat with C weights per point (include/dpr.h, SMOOTH SPLAT, MULTI-CHANNEL): plane
(c, b) is tests/smooth_reference.py for channel c, and the gradients shared by the channels are the sums of its
per-channel gradients.  No arithmetic of its own.  The CPU reference of tests/test_smooth_channels_reference.py and
tests/test_smooth_channels_gpu.py.

Shapes (always batched): points (P, N_in), rotation (B, N_out, N_in), translation (B, N_out), point_weight (P, C),
background (B, C) or None, out_weight (B,) or None; out / ds_dout grid + (C, B).
"""
import numpy as np

from tests import smooth_reference as SR


def raster_smooth_channels(grid, points, rotation, translation, point_weight, background=None, out_weight=None,
                           dtype=np.float64):
    pw = np.asarray(point_weight)
    C = pw.shape[1]
    planes = [SR.raster_smooth(grid, points, rotation, translation,
                               None if background is None else np.asarray(background)[:, c], out_weight, pw[:, c],
                               dtype=dtype) for c in range(C)]
    return np.stack(planes, axis=-2)  # grid + (C, B)


def pullback_parts(ds_dout, points, rotation, translation, point_weight, out_weight=None, dtype=np.float64):
    """The single-channel gradients of every channel: a list of C tuples of tests/smooth_reference.py."""
    g = np.asarray(ds_dout)
    pw = np.asarray(point_weight)
    return [SR.raster_pullback_smooth(g[..., c, :], points, rotation, translation, out_weight, pw[:, c], dtype=dtype)
            for c in range(pw.shape[1])]


def combine(parts):
    """(ds_dpoints (P, N_in), ds_drotation (B, N_out, N_in), ds_dtranslation (B, N_out), ds_dbackground (B, C),
    ds_dout_weight (B,), ds_dpoint_weight (P, C)) of the channels in `parts`."""
    d_pts = sum(p[0] for p in parts)
    d_rot = sum(p[1] for p in parts)
    d_trans = sum(p[2] for p in parts)
    d_bg = np.stack([p[3] for p in parts], axis=-1)
    d_ow = sum(p[4] for p in parts)
    d_pw = np.stack([p[5] for p in parts], axis=-1)
    return d_pts, d_rot, d_trans, d_bg, d_ow, d_pw


def raster_pullback_smooth_channels(ds_dout, points, rotation, translation, point_weight, out_weight=None,
                                    dtype=np.float64):
    return combine(pullback_parts(ds_dout, points, rotation, translation, point_weight, out_weight, dtype=dtype))
