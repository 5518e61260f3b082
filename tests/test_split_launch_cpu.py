"""CPU: how a batch of coalitions is split over engine launches (interpret_quality_amd/engine.py: split_launches, which
CoalitionModel.split_launches and PointNetCls.coalition_logits_wide call), driven through the real model classes with a stub engine
(no library call) and the device's memory figures stubbed.

PointConv's table cache keys on the identity of ``clouds`` / ``centers`` and decides ``walk`` once per batch; a split that sliced
or copied them, or re-derived ``walk`` per launch, would change speed or summation order without failing any shape check."""
import pytest
import torch

from interpret_quality_amd import workspace
from interpret_quality_amd._lib import IqError
from interpret_quality_amd.pointconv import PointConvDensityClsSsg
from interpret_quality_amd.pointnet import PointNetCls
from interpret_quality_amd.pointnet2 import PointNet2ClsMsg

MB = 1 << 20


class _Engine:
    """Records every launch; the 'logits' of a coalition are its keep mask, so the order of the rows can be read back."""
    device = torch.device("cpu")
    _ws = None

    def __init__(self):
        self.launches = []

    def coalition_bytes(self, b, nc, n):
        return b * MB

    def coalition_logits(self, clouds, centers, region_id, keep, cloud_of=None, *extra):
        self.launches.append((clouds, centers, region_id, keep, cloud_of, extra))
        return keep.reshape(-1, 1).float()

    def wide_bytes(self, b, nc, n, r):
        assert r == 128
        return b * MB

    def coalition_logits_wide(self, clouds, centers, region_id, keep, cloud_of=None, num_regions=None):
        assert num_regions == 128 and keep.dim() == 2 and keep.shape[1] == 2
        self.launches.append((clouds, centers, region_id, keep, cloud_of, ()))
        return keep.float()


WIDE = "PointNetCls.coalition_logits_wide"      # the third caller of the splitter: keep rows (b, 2) of a 128-region game
FAMILIES = [PointNet2ClsMsg, PointConvDensityClsSsg, WIDE]


def _run(monkeypatch, cls, nc, b, with_cloud_of, fit):
    monkeypatch.setattr(workspace, "available_bytes", lambda device, held=0: fit * MB)
    wide = cls is WIDE
    if wide:
        monkeypatch.setattr(PointNetCls, "max_wide_per_call", fit)     # 4 where the batch of 10 is to be split
    model = (PointNetCls if wide else cls)(None).eval()
    model._engine = eng = _Engine()
    clouds, centers = torch.zeros((nc, 128, 3)), torch.zeros((nc, 3))
    rid = torch.zeros((nc, 128), dtype=torch.int32)
    keep = torch.arange(b, dtype=torch.int64)
    cloud_of = (torch.arange(b, dtype=torch.int32) % nc).contiguous() if with_cloud_of else None
    if wide:
        keep = torch.stack([keep, keep + 1000], dim=1).contiguous()
        out = model.coalition_logits_wide(clouds, centers, rid, keep, cloud_of, num_regions=128, validate=False)
    else:
        out = model.coalition_logits(clouds, centers, rid, keep, cloud_of, num_regions=32, validate=False)
    assert torch.equal(out.reshape(keep.shape), keep.float())           # every row once, in order
    sizes = [l[3].shape[0] for l in eng.launches]
    assert sum(sizes) == b and max(sizes) <= fit
    lo = 0
    for l in eng.launches:
        assert l[0] is clouds and l[1] is centers and l[2] is rid       # the caller's own tensors on every launch
        assert torch.equal(l[3], keep[lo:lo + l[3].shape[0]]) and l[3].is_contiguous()
        lo += l[3].shape[0]
    return eng.launches, keep, cloud_of


@pytest.mark.parametrize("cls", FAMILIES)
def test_one_source_cloud_needs_no_cloud_of(monkeypatch, cls):
    launches, _, _ = _run(monkeypatch, cls, nc=1, b=10, with_cloud_of=False, fit=4)
    assert [l[3].shape[0] for l in launches] == [4, 4, 2]
    assert all(l[4] is None for l in launches)


@pytest.mark.parametrize("cls", FAMILIES)
def test_one_cloud_per_coalition_is_named_per_launch_only_when_split(monkeypatch, cls):
    launches, _, _ = _run(monkeypatch, cls, nc=10, b=10, with_cloud_of=False, fit=4)
    assert len(launches) == 3
    lo = 0
    for l in launches:
        hi = lo + l[3].shape[0]
        assert l[4].dtype == torch.int32 and l[4].is_contiguous() and torch.equal(l[4], torch.arange(lo, hi, dtype=torch.int32))
        lo = hi
    launches, keep, _ = _run(monkeypatch, cls, nc=10, b=10, with_cloud_of=False, fit=64)
    assert len(launches) == 1 and launches[0][3] is keep and launches[0][4] is None     # unsplit: nothing invented, nothing sliced


@pytest.mark.parametrize("cls", FAMILIES)
def test_callers_cloud_of_is_sliced_with_keep(monkeypatch, cls):
    launches, _, cloud_of = _run(monkeypatch, cls, nc=3, b=10, with_cloud_of=True, fit=4)
    assert len(launches) == 3
    lo = 0
    for l in launches:
        hi = lo + l[3].shape[0]
        assert l[4].is_contiguous() and torch.equal(l[4], cloud_of[lo:hi])
        lo = hi
    launches, keep, cloud_of = _run(monkeypatch, cls, nc=3, b=10, with_cloud_of=True, fit=64)
    assert len(launches) == 1 and launches[0][3] is keep and launches[0][4] is cloud_of


@pytest.mark.parametrize("nc,b,walk", [(1, 10, True), (10, 10, False), (3, 30, True), (8, 10, True), (9, 10, False)])
def test_pointconv_decides_walk_once_from_the_whole_batch(monkeypatch, nc, b, walk):
    launches, _, _ = _run(monkeypatch, PointConvDensityClsSsg, nc, b, with_cloud_of=nc not in (1, b), fit=4)
    assert len(launches) > 1 and all(l[5] == (walk,) for l in launches)
    launches, _, _ = _run(monkeypatch, PointNet2ClsMsg, nc, b, with_cloud_of=nc not in (1, b), fit=4)
    assert all(l[5] == () for l in launches)


@pytest.mark.parametrize("cls", FAMILIES)
def test_several_clouds_without_cloud_of_are_rejected(monkeypatch, cls):
    with pytest.raises(IqError, match="cloud_of is required when 1 < number of clouds != number of coalitions"):
        _run(monkeypatch, cls, nc=3, b=10, with_cloud_of=False, fit=4)
