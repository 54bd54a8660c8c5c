"""numpy restatement of smooth sampling of C-channel images (include/dpr.h, SMOOTH SAMPLING, MULTI-CHANNEL): plane
(c, b) is tests/sample_smooth_reference.py for channel c, and the geometric gradients are the sums of its per-plane
gradients.  No arithmetic of its own.  The CPU reference of tests/test_sample_smooth_channels_reference.py and
tests/test_sample_smooth_channels_gpu.py.

Shapes (always batched): image / ds_dimage grid + (C, B), points (P, N_in), rotation (B, N_out, N_in), translation
(B, N_out); values / ds_dvalues (P, C, B).
"""
import numpy as np

from tests import sample_smooth_reference as SSR


def sample_smooth_channels(image, points, rotation, translation, dtype=np.float64):
    img = np.asarray(image)
    C = img.shape[-2]
    return np.stack([SSR.sample_smooth(img[..., c, :], points, rotation, translation, dtype=dtype) for c in range(C)],
                    axis=1)  # (P, C, B)


def pullback_parts(ds_dvalues, image, points, rotation, translation, dtype=np.float64):
    """The single-plane gradients of every channel: a list of C tuples of tests/sample_smooth_reference.py."""
    img, dv = np.asarray(image), np.asarray(ds_dvalues)
    return [SSR.sample_smooth_pullback(dv[:, c, :], img[..., c, :], points, rotation, translation, dtype=dtype)
            for c in range(img.shape[-2])]


def combine(parts):
    """(ds_dimage grid + (C, B), ds_dpoints (P, N_in), ds_drotation (B, N_out, N_in), ds_dtranslation (B, N_out)) of
    the channels in `parts`."""
    return (np.stack([p[0] for p in parts], axis=-2), sum(p[1] for p in parts), sum(p[2] for p in parts),
            sum(p[3] for p in parts))


def sample_smooth_channels_pullback(ds_dvalues, image, points, rotation, translation, dtype=np.float64):
    return combine(pullback_parts(ds_dvalues, image, points, rotation, translation, dtype=dtype))
