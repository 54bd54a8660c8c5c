"""MI355X-native `raster` / `raster_pullback!` hot path of DiffPointRasterisation.jl.

Exports mirror the reference module (`export raster, raster!, raster_pullback!`,
/root/reference/src/DiffPointRasterisation.jl:17); `!` becomes a trailing underscore.
"""
from . import _lib
from ._lib import DprError, build, lib
from .interface import (ColumnMajorRotation, DimensionMismatch, PullbackResult, column_major_rotation,
                        empty_grid, raster, raster_,
                        raster_pullback_, raster_residual_pullback_, resolve_algo,
                        sharing_effective, sort_points, to_grid_layout, workspace_bytes)
from .timing import stage_times
from .autograd import raster_ad
from .channels import (empty_channel_grid, raster_channels, raster_channels_, raster_channels_ad,
                       raster_pullback_channels_, resolve_algo_channels, workspace_bytes_channels)
from .sample import (SamplePullbackResult, resolve_algo_sample, sample, sample_, sample_ad, sample_pullback_,
                     workspace_bytes_sample)
from .jvp import raster_jvp, raster_jvp_, resolve_algo_jvp, workspace_bytes_jvp
from .clouds import (raster_clouds, raster_clouds_, raster_clouds_ad, raster_pullback_clouds_, resolve_algo_clouds,
                     workspace_bytes_clouds)
from .smooth import (raster_pullback_smooth_, raster_smooth, raster_smooth_, raster_smooth_ad, resolve_algo_smooth,
                     workspace_bytes_smooth)
from .sample_smooth import (resolve_algo_sample_smooth, sample_smooth, sample_smooth_, sample_smooth_ad,
                            sample_smooth_pullback_, workspace_bytes_sample_smooth)
from .smooth_jvp import (raster_smooth_jvp, raster_smooth_jvp_, resolve_algo_smooth_jvp,
                         workspace_bytes_smooth_jvp)
from .smooth_clouds import (raster_pullback_smooth_clouds_, raster_smooth_clouds, raster_smooth_clouds_,
                            raster_smooth_clouds_ad, resolve_algo_smooth_clouds, workspace_bytes_smooth_clouds)
from .smooth_channels import (raster_pullback_smooth_channels_, raster_smooth_channels, raster_smooth_channels_,
                              raster_smooth_channels_ad, resolve_algo_smooth_channels,
                              workspace_bytes_smooth_channels)
from .bodies import (raster_bodies, raster_bodies_, raster_bodies_ad, raster_pullback_bodies_, resolve_algo_bodies)
from .smooth_bodies import (raster_pullback_smooth_bodies_, raster_smooth_bodies, raster_smooth_bodies_,
                            raster_smooth_bodies_ad, resolve_algo_smooth_bodies)
from .smooth_bodies_jvp import (raster_smooth_bodies_jvp, raster_smooth_bodies_jvp_,
                                resolve_algo_smooth_bodies_jvp)
from .sample_smooth_bodies import (resolve_algo_sample_smooth_bodies, sample_smooth_bodies, sample_smooth_bodies_,
                                   sample_smooth_bodies_ad, sample_smooth_bodies_pullback_)
from .sample_smooth_channels import (resolve_algo_sample_smooth_channels, sample_smooth_channels,
                                     sample_smooth_channels_, sample_smooth_channels_ad,
                                     sample_smooth_channels_pullback_)
# (workspace_bytes_sample_smooth_clouds: an attribute of the package, not of `__all__` -- tests/workspace_cases.py
# walks the `workspace_bytes*` names of `__all__`, and this family's plan is the smooth cloud splat's, which it walks)
from .sample_smooth_clouds import (resolve_algo_sample_smooth_clouds, sample_smooth_clouds, sample_smooth_clouds_,
                                   sample_smooth_clouds_ad, sample_smooth_clouds_pullback_,
                                   workspace_bytes_sample_smooth_clouds)
from .sharded import (raster_point_sharded, raster_pullback_point_sharded_,
                      raster_pullback_sharded_, raster_sharded, shard_range)

__all__ = [
    "raster", "raster_", "raster_ad", "raster_pullback_", "raster_residual_pullback_", "PullbackResult",
    "DimensionMismatch", "DprError", "ColumnMajorRotation", "column_major_rotation",
    "empty_grid", "to_grid_layout", "workspace_bytes", "resolve_algo", "sharing_effective", "sort_points", "build", "lib",
    "stage_times", "raster_sharded", "raster_pullback_sharded_", "shard_range",
    "raster_point_sharded", "raster_pullback_point_sharded_",
    "raster_channels", "raster_channels_", "raster_pullback_channels_", "raster_channels_ad", "empty_channel_grid",
    "resolve_algo_channels", "workspace_bytes_channels",
    "sample", "sample_", "sample_pullback_", "sample_ad", "SamplePullbackResult", "resolve_algo_sample",
    "workspace_bytes_sample",
    "raster_jvp", "raster_jvp_", "resolve_algo_jvp", "workspace_bytes_jvp",
    "raster_clouds", "raster_clouds_", "raster_pullback_clouds_", "raster_clouds_ad", "resolve_algo_clouds",
    "workspace_bytes_clouds",
    "raster_smooth", "raster_smooth_", "raster_pullback_smooth_", "raster_smooth_ad", "resolve_algo_smooth",
    "workspace_bytes_smooth",
    "sample_smooth", "sample_smooth_", "sample_smooth_pullback_", "sample_smooth_ad", "resolve_algo_sample_smooth",
    "workspace_bytes_sample_smooth",
    "raster_smooth_jvp", "raster_smooth_jvp_", "resolve_algo_smooth_jvp", "workspace_bytes_smooth_jvp",
    "raster_smooth_clouds", "raster_smooth_clouds_", "raster_pullback_smooth_clouds_", "raster_smooth_clouds_ad",
    "resolve_algo_smooth_clouds", "workspace_bytes_smooth_clouds",
    "raster_smooth_channels", "raster_smooth_channels_", "raster_pullback_smooth_channels_",
    "raster_smooth_channels_ad", "resolve_algo_smooth_channels", "workspace_bytes_smooth_channels",
    "raster_bodies", "raster_bodies_", "raster_pullback_bodies_", "raster_bodies_ad", "resolve_algo_bodies",
    "raster_smooth_bodies", "raster_smooth_bodies_", "raster_pullback_smooth_bodies_", "raster_smooth_bodies_ad",
    "resolve_algo_smooth_bodies",
    "raster_smooth_bodies_jvp", "raster_smooth_bodies_jvp_", "resolve_algo_smooth_bodies_jvp",
    "sample_smooth_bodies", "sample_smooth_bodies_", "sample_smooth_bodies_pullback_", "sample_smooth_bodies_ad",
    "resolve_algo_sample_smooth_bodies",
    "sample_smooth_channels", "sample_smooth_channels_", "sample_smooth_channels_pullback_",
    "sample_smooth_channels_ad", "resolve_algo_sample_smooth_channels",
    "sample_smooth_clouds", "sample_smooth_clouds_", "sample_smooth_clouds_pullback_", "sample_smooth_clouds_ad",
    "resolve_algo_sample_smooth_clouds",
]
