"""The reference's `models.*` import path resolves to this build (no GPU needed): every module-level name the reference's
scripts import from models/pointnet.py, pointnet2.py, dgcnn.py and pointconv.py, the classifier classes being the HIP-backed
classes themselves, the training-only building blocks absent, and the kNN's limits checked before any device is touched."""
import importlib

import pytest
import torch

SURFACE = {
    "models.pointnet": "PointNetCls",
    "models.pointnet2": "PointNet2ClsMsg square_distance index_points farthest_point_sample query_ball_point sample_and_group "
                        "sample_and_group_all",
    "models.dgcnn": "DGCNN_cls GCNN_cls knn get_graph_feature",
    "models.pointconv": "PointConvDensityClsSsg square_distance index_points farthest_point_sample query_ball_point knn_point "
                        "sample_and_group sample_and_group_all group compute_density",
}

OUT_OF_SCOPE = {
    "models.pointnet": "STNkd PointNetfeat feature_transform_regularizer",
    "models.pointnet2": "PointNetSetAbstraction PointNetSetAbstractionMsg timeit",
    "models.dgcnn": "",
    "models.pointconv": "DensityNet WeightNet PointConvSetAbstraction PointConvDensitySetAbstraction timeit",
}


@pytest.mark.parametrize("mod", sorted(SURFACE))
def test_reference_names_importable(mod):
    m = importlib.import_module(mod)
    missing = [n for n in SURFACE[mod].split() if not hasattr(m, n)]
    assert not missing, (mod, missing)
    assert all(callable(getattr(m, n)) for n in SURFACE[mod].split())


def test_classes_are_the_hip_backed_classes():
    from interpret_quality_amd import dgcnn, final_util, pointconv, pointnet, pointnet2
    import models.dgcnn
    import models.pointconv
    import models.pointnet
    import models.pointnet2
    assert models.pointnet.PointNetCls is pointnet.PointNetCls
    assert models.pointnet2.PointNet2ClsMsg is pointnet2.PointNet2ClsMsg
    assert models.dgcnn.DGCNN_cls is dgcnn.DGCNN_cls and models.dgcnn.GCNN_cls is dgcnn.GCNN_cls
    assert models.pointconv.PointConvDensityClsSsg is pointconv.PointConvDensityClsSsg
    assert models.pointnet2.square_distance is final_util.square_distance
    assert models.pointconv.square_distance is final_util.square_distance


@pytest.mark.parametrize("mod", sorted(OUT_OF_SCOPE))
def test_training_building_blocks_are_absent(mod):
    m = importlib.import_module(mod)
    present = [n for n in OUT_OF_SCOPE[mod].split() if hasattr(m, n)]
    assert not present, (mod, present)


@pytest.mark.parametrize("shape,k,what", [((2, 3, 64), 10, "k=10"), ((2, 5, 64), 20, "C=5"), ((2, 3, 100), 20, "N=100")])
def test_knn_limits_raise_value_error_before_any_device(shape, k, what):
    """Outside iq_knn's limits (k = 20, C in {3, 64, 128}, N % 32 == 0) there is no fallback: ValueError naming the limit,
    raised for a CPU tensor too, i.e. before anything reaches a device."""
    from models.dgcnn import get_graph_feature, knn
    x = torch.zeros(shape)
    with pytest.raises(ValueError, match=what):
        knn(x, k)
    with pytest.raises(ValueError, match=what):
        get_graph_feature(x, k=k)
