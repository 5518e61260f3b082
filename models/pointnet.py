"""models/pointnet.py of the reference: the classifier (the nn building blocks are training code, not provided)."""
from interpret_quality_amd.pointnet import PointNetCls

__all__ = ["PointNetCls"]
