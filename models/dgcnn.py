"""models/dgcnn.py of the reference: DGCNN_cls, GCNN_cls, knn and get_graph_feature on the HIP ops."""
from interpret_quality_amd import hip_ops
from interpret_quality_amd.dgcnn import DGCNN_cls, GCNN_cls

__all__ = ["DGCNN_cls", "GCNN_cls", "knn", "get_graph_feature"]

KNN_K = 20
KNN_CHANNELS = (3, 64, 128)


def _check_knn_limits(x, k):
    """iq_knn's limits, checked before anything touches a device: there is no fallback outside them."""
    if k != KNN_K:
        raise ValueError("knn: k=%d, the HIP kNN (iq_knn) supports k = %d only" % (k, KNN_K))
    if x.dim() != 3:
        raise ValueError("knn: x must be (B,C,N), got %d dims" % x.dim())
    if x.shape[1] not in KNN_CHANNELS:
        raise ValueError("knn: C=%d, the HIP kNN (iq_knn) supports C in %s" % (x.shape[1], KNN_CHANNELS))
    if x.shape[2] % 32:
        raise ValueError("knn: N=%d, the HIP kNN (iq_knn) needs N to be a multiple of 32" % x.shape[2])


def knn(x, k):
    """models/dgcnn.py:12-18: x (B,C,N) -> (B,N,k) long, the k nearest rows (self included) nearest first
    (iq_knn for the set, iq_sort_neighbours for topk's order)."""
    _check_knn_limits(x, k)
    xt = x.transpose(2, 1).contiguous()
    idx = hip_ops.knn(xt, k)
    return hip_ops.sort_neighbours(xt, xt, idx).long()


def get_graph_feature(x, k=20, idx=None, dim9=False):
    """models/dgcnn.py:21-47: x (B,C,N) -> (B,2C,N,k) edge features [x_j - x_i ; x_i] (iq_edgeconv_gather)."""
    b, n = x.size(0), x.size(2)
    x = x.view(b, -1, n)
    if idx is None:
        idx = knn(x if not dim9 else x[:, 6:], k=k)
    return hip_ops.edgeconv_gather(x.contiguous(), idx, channel_first=True)
