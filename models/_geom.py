"""The geometric helpers the reference's model files share, on the HIP ops (interpret_quality_amd.hip_ops)."""
import torch

from interpret_quality_amd import hip_ops


def index_points(points, idx):
    """models/pointnet2.py:27-43 = models/pointconv.py:35-52: points (B,N,C), idx (B,D1,..,Dn) -> (B,D1,..,Dn,C)."""
    return hip_ops.index_points(points.contiguous(), idx)


def farthest_point_sample(xyz, npoint):
    """models/pointnet2.py:45-68 = models/pointconv.py:54-77: xyz (B,N,3) -> (B,npoint) long (iq_fps)."""
    return hip_ops.fps(xyz.contiguous(), npoint).long()


def query_ball_point(radius, nsample, xyz, new_xyz):
    """models/pointnet2.py:70-91 = models/pointconv.py:79-100: (B,S,nsample) long (iq_ball_query)."""
    return hip_ops.ball_query(xyz.contiguous(), new_xyz.contiguous(), radius, nsample).long()


def knn_point(nsample, xyz, new_xyz):
    """models/pointconv.py:103-114: the nsample nearest points of every query, (B,S,nsample) long.  The reference returns the
    set unsorted; this one is sorted nearest first, ties to the lower index (iq_knn_point)."""
    return hip_ops.knn_point(xyz.contiguous(), new_xyz.contiguous(), nsample).long()


def group(xyz, points, new_xyz, idx, xyz_first=True):
    """[xyz[idx] - new_xyz, points[idx]] (or features first) as one gather (iq_group_points); idx None: all points."""
    return hip_ops.group_points(xyz.contiguous(), points.contiguous() if points is not None else None,
                                new_xyz.contiguous() if new_xyz is not None else None, idx, xyz_first)


def device_zeros(b, c, like):
    return torch.zeros(b, 1, c, dtype=like.dtype, device=like.device)
