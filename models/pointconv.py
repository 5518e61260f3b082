"""models/pointconv.py of the reference: PointConvDensityClsSsg and the module-level geometric helpers on the HIP ops."""
from interpret_quality_amd import hip_ops
from interpret_quality_amd.final_util import square_distance
from interpret_quality_amd.pointconv import PointConvDensityClsSsg

from ._geom import farthest_point_sample, group as _group, index_points, knn_point, query_ball_point

__all__ = ["PointConvDensityClsSsg", "square_distance", "index_points", "farthest_point_sample", "query_ball_point",
           "knn_point", "sample_and_group", "sample_and_group_all", "group", "compute_density"]


def sample_and_group(npoint, nsample, xyz, points, density_scale=None):
    """models/pointconv.py:117-145: new_xyz, new_points (B,S,K,3+D), grouped_xyz_norm (B,S,K,3), idx [, grouped_density]."""
    new_xyz = index_points(xyz, farthest_point_sample(xyz, npoint))
    idx = knn_point(nsample, xyz, new_xyz)
    grouped_xyz_norm = _group(xyz, None, new_xyz, idx)
    new_points = _group(xyz, points, new_xyz, idx) if points is not None else grouped_xyz_norm
    if density_scale is None:
        return new_xyz, new_points, grouped_xyz_norm, idx
    return new_xyz, new_points, grouped_xyz_norm, idx, index_points(density_scale, idx)


def sample_and_group_all(xyz, points, density_scale=None):
    """models/pointconv.py:148-171: new_xyz = the mean point (B,1,3), new_points (B,1,N,3+D) = [xyz - mean, points]."""
    b, n, c = xyz.shape
    new_xyz = xyz.mean(dim=1, keepdim=True)
    grouped_xyz = _group(xyz, None, new_xyz, None)
    new_points = _group(xyz, points, new_xyz, None) if points is not None else grouped_xyz
    if density_scale is None:
        return new_xyz, new_points, grouped_xyz
    return new_xyz, new_points, grouped_xyz, density_scale.view(b, 1, n, 1)


def group(nsample, xyz, points):
    """models/pointconv.py:174-197: the nsample nearest neighbours of every point -> new_points, grouped_xyz_norm."""
    idx = knn_point(nsample, xyz, xyz)
    grouped_xyz_norm = _group(xyz, None, xyz, idx)
    new_points = _group(xyz, points, xyz, idx) if points is not None else grouped_xyz_norm
    return new_points, grouped_xyz_norm


def compute_density(xyz, bandwidth):
    """models/pointconv.py:199-209: Gaussian kernel density of every point, (B,N) (iq_density)."""
    return hip_ops.density(xyz.contiguous(), bandwidth)
