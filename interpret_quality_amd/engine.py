"""What the four model families share above the C ABI: packing folded weights for the library, the engine that owns them and a
workspace and issues the launches, and the ``nn.Module`` side that splits a batch of coalitions over launches.

A family module keeps what is its own: the architecture constants, the walk over the state dict that fills its ctypes struct
(with its own rule for which layers are ALSO packed as three bf16 terms - the rule decides which kernel a layer runs on), the
workspace-size and launch calls of the library, and its specials.
"""
import numpy as np
import torch

from . import _lib, hip_ops, workspace

BN_EPS = 1e-5


def _np(t):
    return t.detach().cpu().double().numpy()


def bn_scale(sd, bn):
    return _np(sd[bn + ".weight"]) / np.sqrt(_np(sd[bn + ".running_var"]) + BN_EPS)


def bn_affine(sd, bn):
    """Eval-mode BatchNorm as y = s.x + t, float64."""
    s = bn_scale(sd, bn)
    return s, _np(sd[bn + ".bias"]) - _np(sd[bn + ".running_mean"]) * s


def fold(sd, layer, bn):
    """(W (cout,cin), b) of ``bn(layer(x))`` in eval mode, float64; ``Packer.dense`` rounds once to float32."""
    w = _np(sd[layer + ".weight"])
    w = w.reshape(w.shape[0], -1)
    b = _np(sd[layer + ".bias"])
    if bn is not None:
        s = bn_scale(sd, bn)
        w = w * s[:, None]
        b = (b - _np(sd[bn + ".running_mean"])) * s + _np(sd[bn + ".bias"])
    return w, b


class Packer:
    """Base of the families' PackedWeights*: uploads arrays to ``device`` and keeps them alive for the ctypes struct."""

    def __init__(self, device):
        self.lib = _lib.load()
        self.device = device
        self._keep = []

    def dev(self, arr, dtype=np.float32):
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).to(self.device)
        self._keep.append(t)
        return t

    def bf3(self, w):
        """The same folded weights as three bf16 terms on the device (products on the bf16 matrix pipe, float32-exact)."""
        cout, cin = w.shape
        w32 = np.ascontiguousarray(w, dtype=np.float32)
        out = np.empty(self.lib.iq_packed_bf3_elems(cout, cin), dtype=np.uint16)
        _lib.check(self.lib.iq_pack_weight_bf3(w32.ctypes.data, out.ctypes.data, cout, cin), "iq_pack_weight_bf3")
        return self.dev(out.view(np.int16), np.int16).data_ptr()

    def dense(self, w, b, bf3=False):
        """Fragment-packed weights + padded bias as an iq_dense_layer; ``bf3``: the family's decision to fill w_bf3 too."""
        cout, cin = w.shape
        w32 = np.ascontiguousarray(w, dtype=np.float32)
        out = np.empty(self.lib.iq_packed_floats(cout, cin), dtype=np.float32)
        _lib.check(self.lib.iq_pack_weight(w32.ctypes.data, out.ctypes.data, cout, cin), "iq_pack_weight")
        bp = np.zeros(self.lib.iq_padded_cout(cout), dtype=np.float32)
        bp[:cout] = b
        wt, bt = self.dev(out), self.dev(bp)
        return _lib.DenseLayer(wt.data_ptr(), bt.data_ptr(), cin, cout, self.bf3(w32) if bf3 else None)


ptr, stream = hip_ops._p, hip_ops._stream      # tensor or None -> void pointer; the current stream


def check_coalition_args(clouds, centers, region_id, keep, cloud_of, masked=True):
    """``masked=False`` (PointNet's dense forward through its coalition entry): centers and keep may be None, like cloud_of.
    The required tensors are checked first, then the optional ones."""
    args = ((clouds, torch.float32, "clouds", True), (centers, torch.float32, "centers", masked),
            (region_id, torch.int32, "region_id", True), (keep, torch.int64, "keep", masked), (cloud_of, torch.int32, "cloud_of", False))
    for required in (True, False):
        for t, dt, nm, req in args:
            if req != required or (t is None and not req):
                continue
            if t is None or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise _lib.IqError("%s must be a contiguous %s GPU tensor" % (nm, dt))


class Engine:
    """Owns a family's packed weights (``packed``: its PackedWeights* class) and one growable workspace, and issues the launches.
    A family gives the workspace sizes (``forward_bytes``, ``coalition_bytes``) and the two library calls (``_forward``,
    ``_coalitions``, each returning the status code)."""
    packed = None

    def __init__(self, state_dict, device, *packer_args):
        if torch.device(device).type != "cuda":
            raise _lib.IqError("%s needs a GPU device (no CPU fallback)" % type(self).__name__)
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.weights = self.packed(state_dict, self.device, *packer_args)
        self._ws = None

    def workspace_replaced(self):
        """workspace.ensure calls this between dropping the old workspace and allocating the new one."""

    def new_logits(self, b):
        return torch.empty((b, self.weights.num_classes), dtype=torch.float32, device=self.device)

    def forward_points(self, xyz):
        """xyz (B,N,3) contiguous float32 on the GPU -> logits (B,C)."""
        if not xyz.is_cuda or xyz.dtype != torch.float32 or not xyz.is_contiguous():
            raise _lib.IqError("xyz must be a contiguous float32 GPU tensor (B,N,3)")
        b, n, _ = xyz.shape
        ws = workspace.ensure(self, self.forward_bytes(b, n))
        logits = self.new_logits(b)
        _lib.check(self._forward(xyz, logits, ws, b, n), self.forward_name)
        return logits

    def coalition_logits(self, clouds, centers, region_id, keep, cloud_of=None, *extra):
        """clouds (nc,N,3), centers (nc,3), region_id (nc,N) i32, keep (B,) i64 bit masks, cloud_of (B,) i32 or None -> logits
        (B,C).  The masked clouds are written inside the library or never.  ``extra``: the family's per-batch arguments."""
        check_coalition_args(clouds, centers, region_id, keep, cloud_of)
        nc, n, _ = clouds.shape
        b = keep.shape[0]
        ws = workspace.ensure(self, self.coalition_bytes(b, nc, n))
        logits = self.new_logits(b)
        _lib.check(self._coalitions(clouds, centers, region_id, keep, cloud_of, logits, ws, b, nc, n, *extra), self.coalitions_name)
        return logits

    def coalition_logits_wide(self, clouds, centers, region_id, keep, cloud_of=None, num_regions=None, *extra):
        """``coalition_logits`` for a game of up to hip_ops.MAX_WIDE_REGIONS regions: keep (B,W) int64 rows, W = ceil(R / 64), bit
        (r & 63) of word (r >> 6) = region r kept - one launch of the family's ``_coalitions_wide``.  The same workspace as the
        narrow launch: only the kernels that read a mask differ (include/iq.h, "Wide coalitions")."""
        check_coalition_args(clouds, centers, region_id, keep, cloud_of)
        r = int(num_regions)
        hip_ops.wide_keep(keep, r)
        nc, n, _ = clouds.shape
        b = keep.shape[0]
        ws = workspace.ensure(self, self.coalition_bytes(b, nc, n))
        logits = self.new_logits(b)
        _lib.check(self._coalitions_wide(clouds, centers, region_id, keep, cloud_of, logits, ws, b, nc, n, r, *extra),
                   self.coalitions_name + "_wide")
        return logits


class EngineOwner:
    """``nn.Module`` mixin: the engine (packed image of the parameters) is built on first use and dropped on any parameter change.
    A family gives ``eval_only`` (the message) and ``_new_engine()``."""
    _engine = None

    def load_state_dict(self, *a, **k):
        self._engine = None
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    def engine(self):
        if self.training:
            raise _lib.IqError(self.eval_only)
        if self._engine is None:
            self._engine = self._new_engine()
        return self._engine


class CoalitionModel(EngineOwner):
    """The families whose launches are sized from the memory that is free (workspace.run_in_steps), at most
    ``max_clouds_per_call`` clouds each."""

    def forward_points(self, xyz):
        """(B,N,3) channel-last clouds (what the mask kernel writes) -> logits."""
        eng = self.engine()
        total, n = xyz.shape[0], xyz.shape[1]
        return workspace.run_in_steps(eng, total, self.max_clouds_per_call, lambda b: eng.forward_bytes(b, n),
                                      lambda lo, hi: eng.forward_points(xyz if (lo, hi) == (0, total) else xyz[lo:hi].contiguous()))

    def forward(self, xyz):
        """xyz (B,3,N) as in the reference -> logits (B,10)."""
        return self.forward_points(xyz.permute(0, 2, 1).contiguous())

    def coalition_logits(self, clouds, centers, region_id, keep, cloud_of=None, num_regions=None, validate=True):
        """Same call as PointNetCls.coalition_logits: logits of B coalitions given as region bit masks.  ``validate``: check
        region_id against [0, num_regions) first (one stream sync); the drivers validate the ids once per cloud on the host and
        pass False."""
        if validate:
            hip_ops.check_index_range(region_id, 0, int(num_regions) if num_regions else 64, "region_id")
        return self.split_launches(self.engine(), clouds, centers, region_id, keep, cloud_of)

    def split_launches(self, eng, clouds, centers, region_id, keep, cloud_of, *extra):
        """``split_launches`` over eng.coalition_logits, at most ``max_clouds_per_call`` coalitions a launch; every launch gets the
        same ``extra``."""
        nc, n = clouds.shape[0], clouds.shape[1]
        return split_launches(eng, lambda k, names: eng.coalition_logits(clouds, centers, region_id, k, names, *extra),
                              lambda k: eng.coalition_bytes(k, nc, n), self.max_clouds_per_call, clouds, keep, cloud_of)

    def coalition_logits_wide(self, clouds, centers, region_id, keep, cloud_of=None, num_regions=None, validate=True):
        """``coalition_logits`` for wide coalitions: keep (B,W) int64 rows over ``num_regions`` <= hip_ops.MAX_WIDE_REGIONS regions
        (one region per point included), through the family's compact path.  For 64 regions and fewer the logits are
        ``coalition_logits``'s on the same masks, bit for bit; above, they are its bits on the same kept points."""
        r = int(num_regions)
        hip_ops.wide_keep(keep, r)
        if validate:
            hip_ops.check_index_range(region_id, 0, r, "region_id")
        return self.split_launches_wide(self.engine(), clouds, centers, region_id, keep, cloud_of, r)

    def split_launches_wide(self, eng, clouds, centers, region_id, keep, cloud_of, r, *extra):
        """``split_launches`` over eng.coalition_logits_wide: the same cap and the same workspace sizes as the narrow launches."""
        nc, n = clouds.shape[0], clouds.shape[1]
        return split_launches(eng, lambda k, names: eng.coalition_logits_wide(clouds, centers, region_id, k, names, r, *extra),
                              lambda k: eng.coalition_bytes(k, nc, n), self.max_clouds_per_call, clouds, keep, cloud_of)


def check_cloud_of(clouds, keep, cloud_of):
    if cloud_of is None and clouds.shape[0] not in (1, keep.shape[0]):
        raise _lib.IqError("cloud_of is required when 1 < number of clouds != number of coalitions")


def split_launches(eng, launch_fn, bytes_fn, cap, clouds, keep, cloud_of):
    """``launch_fn(keep, cloud_of) -> logits`` in one engine launch if the workspace fits, several otherwise: the launch size
    comes from the memory that is free now (workspace.run_in_steps, ``bytes_fn(coalitions)``), at most ``cap``.  Only ``keep`` and
    ``cloud_of`` are sliced - ``launch_fn`` passes the caller's own ``clouds``, ``centers`` and ``region_id`` tensors on every launch
    (an engine may key a cache on their identity).  ``keep`` is whatever has one row per unit of ``cap``, ``bytes_fn`` and
    ``cloud_of``: keep masks or rows (a unit is a coalition) or permutations (PointNet's prefix route: a unit is a permutation,
    and a launch returns R + 1 rows for each)."""
    check_cloud_of(clouds, keep, cloud_of)
    nc, b = clouds.shape[0], keep.shape[0]
    names = cloud_of

    def call(lo, hi):
        nonlocal names
        if (lo, hi) == (0, b):
            return launch_fn(keep, cloud_of)
        if names is None and nc == b:      # one cloud per coalition, split over launches: name each launch's clouds
            names = torch.arange(b, dtype=torch.int32, device=keep.device)
        return launch_fn(keep[lo:hi].contiguous(), names[lo:hi].contiguous() if names is not None else None)
    return workspace.run_in_steps(eng, b, cap, bytes_fn, call)
