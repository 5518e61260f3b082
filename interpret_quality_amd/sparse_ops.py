"""The wrappers of the sparse regression control variate (include/iq.h, "Sparse regression control variate"; DESIGN.md 5k;
csrc/iq_kshap_sparsecv.hip): a 2-additive surrogate of all R singles and a listed K pairs, d = R + K <= 2080, on FEATURE ROWS -
row m of the keep rows expanded into its d feature bits, (M, ceil(d / 64)) int64-typed.

Like the control-variate wrappers of hip_ops.py these lend the library ZEROED memory only: what a call returns cannot depend on
an earlier call's bytes whatever a kernel reads (tests/test_kshap_sparse_gpu.py hands the same calls hostile memory between guard
zones and asks for the same bits).  A missing kernel is an error: there is no fall-back."""
import numpy as np
import torch

from . import _lib, hip_ops
from .hip_ops import KshapSingular, _dev, _opt, _p, _shape, _stream

MAX_FEATURES = 2080        # IQ_KSHAP_SPARSE_MAX_FEATURES of include/iq.h


def check_pair_list(pairs, r):
    """A pair list by the contract -> (K,2) int32 C-contiguous ndarray: 0 <= i < j < r, strictly increasing in row-major order
    (so no duplicates), r + K <= MAX_FEATURES.  IqError otherwise, before anything is launched."""
    r = hip_ops.kshap_regions_wide(r)
    if isinstance(pairs, torch.Tensor):
        pairs = pairs.cpu().numpy()
    p = np.asarray(pairs)
    if p.size == 0:
        p = np.zeros((0, 2), dtype=np.int32)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu":
        raise _lib.IqError("a pair list must be (K,2) integers, got shape %s of %s" % (tuple(p.shape), p.dtype))
    p = p.astype(np.int64)
    k = p.shape[0]
    if r + k > MAX_FEATURES:
        raise _lib.IqError("a sparse surrogate has at most %d features: %d regions leave %d pairs, got %d"
                           % (MAX_FEATURES, r, MAX_FEATURES - r, k))
    ok = (p[:, 0] >= 0) & (p[:, 0] < p[:, 1]) & (p[:, 1] < r)
    if not ok.all():
        bad = int(np.argmin(ok))
        raise _lib.IqError("a pair list holds pairs (i, j) with 0 <= i < j < %d: row %d is %s" % (r, bad, p[bad].tolist()))
    rising = np.diff(p[:, 0] * r + p[:, 1]) > 0
    if not rising.all():
        bad = int(np.argmin(rising))
        raise _lib.IqError("a pair list is strictly increasing in row-major order (sorted, no duplicates): row %d is not above row %d"
                           % (bad + 1, bad))
    return np.ascontiguousarray(p.astype(np.int32))


def feature_words(d):
    """Words per feature row: ceil(d / 64), 2 <= d <= MAX_FEATURES."""
    d = int(d)
    if not 2 <= d <= MAX_FEATURES:
        raise _lib.IqError("a sparse surrogate has 2 .. %d features, got %d" % (MAX_FEATURES, d))
    return (d + 63) // 64


def _rows(m, what):
    if not 1 <= m <= 1 << 30:
        raise _lib.IqError("%s: M=%d rows is out of range" % (what, m))


def _feat(feat, d, what):
    """Feature rows (M, ceil(d / 64)) int64 on the device -> (pointer, M)."""
    wd = feature_words(d)
    if not isinstance(feat, torch.Tensor) or feat.dim() != 2 or feat.shape[1] != wd:
        raise _lib.IqError("%s: feat must be (M, %d) for %d features, got %s"
                           % (what, wd, int(d), tuple(feat.shape) if isinstance(feat, torch.Tensor) else type(feat).__name__))
    _rows(feat.shape[0], what)
    return _dev(feat, torch.int64, "feat"), feat.shape[0]


def kshap_sparse_expand(keep, pairs, r):
    """keep (M,) narrow or (M,W) wide rows, pairs a pair list (``check_pair_list``) -> feat (M, ceil((r + K) / 64)) int64-typed:
    bit a of row m = f_a(S_m), the singles first, then the listed pairs in list order (iq_kshap_sparse_expand).  Bits of keep at
    or above r are ignored, bits of feat at or above r + K are 0."""
    lib = _lib.load()
    p = check_pair_list(pairs, r)
    r = int(r)
    kp, m = hip_ops._sampled_rows(keep, r)
    _rows(m, "kshap_sparse_expand")
    k = p.shape[0]
    dev = keep.device
    plist = torch.from_numpy(p).to(dev) if k else None
    feat = torch.zeros((m, feature_words(r + k)), dtype=torch.int64, device=dev)
    _lib.check(lib.iq_kshap_sparse_expand(kp, _p(plist), m, r, k, _p(feat), _stream()), "iq_kshap_sparse_expand")
    return feat


def kshap_feat_gram(feat, d):
    """feat (M, Wd) feature rows -> (d,d) f64: Gram[a][b] = the number of rows that hold features a and b, exact counts
    (iq_kshap_feat_gram: the d x d x M product on the f64 matrix pipe; bits at or above d are ignored)."""
    lib = _lib.load()
    fp, m = _feat(feat, d, "kshap_feat_gram")
    d = int(d)
    gram = torch.zeros((d, d), dtype=torch.float64, device=feat.device)
    _lib.check(lib.iq_kshap_feat_gram(fp, m, d, _p(gram), _stream()), "iq_kshap_feat_gram")
    return gram


def kshap_feat_fit(gram, feat, v, v0, delta, d, ridge, solves=False):
    """gram (d,d) of ``kshap_feat_gram`` on the same rows, feat (M,Wd), v (G,M) f32, v0 and delta (G,) f64, ridge >= 0 -> beta (G,d)
    f64: hip_ops.kshap_pair_fit on feature rows (iq_kshap_feat_fit: the same factor, solve and constrain kernels).  ``solves``:
    -> (beta, (G+1,d) f64).  KshapSingular when a pivot fails (a status word read back)."""
    lib = _lib.load()
    fp, m = _feat(feat, d, "kshap_feat_fit")
    d = int(d)
    _shape(gram, "gram", d, d)
    g, _ = _shape(v, "v", None, m)
    _shape(v0, "v0", g)
    _shape(delta, "delta", g)
    ridge = float(ridge)
    if not ridge >= 0.0:
        raise _lib.IqError("kshap_feat_fit: ridge must be a number >= 0, got %r" % ridge)
    dev = feat.device
    nbytes = lib.iq_kshap_feat_fit_scratch_bytes(m, d, g)
    scratch = torch.zeros((hip_ops._kshap_scratch_words("kshap_feat_fit", nbytes, m, d, g, "d"),), dtype=torch.float64, device=dev)
    beta = torch.zeros((g, d), dtype=torch.float64, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    both = torch.zeros((g + 1, d), dtype=torch.float64, device=dev) if solves else None
    _lib.check(lib.iq_kshap_feat_fit(_dev(gram, torch.float64, "gram"), fp, _dev(v, torch.float32, "v"), _dev(v0, torch.float64, "v0"),
                                     _dev(delta, torch.float64, "delta"), ridge, m, d, g, _p(beta), _p(both), _p(status), _p(scratch),
                                     nbytes, _stream()), "iq_kshap_feat_fit")
    if int(status.item()):
        raise KshapSingular("the rows do not determine the sparse surrogate (%d rows, %d unknowns, ridge %g): draw more samples, "
                            "list fewer pairs or use a ridge > 0" % (m, d, ridge))
    return (beta, both) if solves else beta


def kshap_feat_surrogate(feat, beta, d, v=None, v0=None):
    """feat (M,Wd), beta (G,d) f64 -> g (G,M) f64, g[g][m] = the sum of beta[g] over the features row m holds, in index order
    (iq_kshap_feat_surrogate).  With v (G,M) f32 and v0 (G,) f64: -> (g, t), t = ((double)v - v0) - g, the residual terms."""
    lib = _lib.load()
    fp, m = _feat(feat, d, "kshap_feat_surrogate")
    d = int(d)
    g, _ = _shape(beta, "beta", None, d)
    dev = feat.device
    out = torch.zeros((g, m), dtype=torch.float64, device=dev)
    t = None
    if v is not None:
        _shape(v, "v", g, m)
        _shape(v0, "v0", g)
        t = torch.zeros((g, m), dtype=torch.float64, device=dev)
    _lib.check(lib.iq_kshap_feat_surrogate(fp, _dev(beta, torch.float64, "beta"), _opt(v if t is not None else None, torch.float32, "v"),
                                           _opt(v0 if t is not None else None, torch.float64, "v0"), m, d, g, _p(out), _p(t),
                                           _stream()), "iq_kshap_feat_surrogate")
    return out if t is None else (out, t)
