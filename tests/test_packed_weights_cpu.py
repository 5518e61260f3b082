"""CPU: every byte the four families hand to the library is what it was before the host layer was consolidated.

``PackedWeights*`` accept ``device="cpu"`` (the packing routines of libiq_hip.so are host code), so the whole image can be
fingerprinted without a GPU: the ctypes struct is walked recursively; a scalar field contributes its value, a pointer field the
dtype, shape and sha256 of the ``_keep`` tensor whose ``data_ptr()`` it equals (NULL stays NULL; a pointer that matches no kept
tensor is an error); then ``num_classes``, the number of kept tensors and, for PointNet, ``feature_transform`` and the bytes of
``unpack_index``.

tests/golden/packed_weights.json was recorded with ``fingerprint`` below at commit 679b5f9 ("PointNet chain kernel: layers 2-3
on v_mfma_f32_16x16x32_bf16"), the last one in which each family module packed its own weights - never from the code under
test.  A difference here changes which kernel a layer runs on or the bits of its weights, hence the logits.
"""
import ctypes
import hashlib
import json
import os

import pytest

from interpret_quality_amd import synth
from interpret_quality_amd.dgcnn import PackedWeightsD
from interpret_quality_amd.pointconv import PackedWeightsC
from interpret_quality_amd.pointnet import PackedWeights
from interpret_quality_amd.pointnet2 import PackedWeights2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_weights.json")

CASES = {
    "pointnet": lambda: PackedWeights(synth.to_torch(synth.pointnet_state_dict(0)), "cpu"),
    "pointnet_noft": lambda: PackedWeights(synth.to_torch(synth.pointnet_state_dict(0, feature_transform=False)), "cpu"),
    "pointnet2": lambda: PackedWeights2(synth.to_torch(synth.pointnet2_state_dict(0)), "cpu"),
    "pointconv": lambda: PackedWeightsC(synth.to_torch(synth.pointconv_state_dict(0)), "cpu"),
    "dgcnn": lambda: PackedWeightsD(synth.to_torch(synth.dgcnn_state_dict(0)), "cpu", 20),
}


def _tensor_record(t):
    data = t.detach().cpu().contiguous().numpy().tobytes()
    return {"dtype": str(t.dtype), "shape": list(t.shape), "sha256": hashlib.sha256(data).hexdigest()}


def _walk(value, ctype, kept, path):
    if issubclass(ctype, ctypes.Structure):
        return {name: _walk(getattr(value, name), ft, kept, path + "." + name) for name, ft in ctype._fields_}
    if issubclass(ctype, ctypes.Array):
        return [_walk(value[i], ctype._type_, kept, "%s[%d]" % (path, i)) for i in range(ctype._length_)]
    if ctype is ctypes.c_void_p:
        if not value:
            return None
        assert value in kept, "%s points at no kept tensor" % path
        return _tensor_record(kept[value])
    return value


def fingerprint(pw):
    kept = {t.data_ptr(): t for t in pw._keep}
    assert len(kept) == len(pw._keep)
    rec = {"struct": _walk(pw.struct, type(pw.struct), kept, type(pw.struct).__name__),
           "num_classes": pw.num_classes, "kept_tensors": len(pw._keep)}
    if hasattr(pw, "unpack_index"):
        rec["feature_transform"] = bool(pw.feature_transform)
        rec["unpack_index"] = _tensor_record(pw.unpack_index)
    return rec


@pytest.mark.parametrize("case", sorted(CASES))
def test_packed_image_is_the_recorded_one(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = json.loads(json.dumps(fingerprint(CASES[case]())))      # floats and lists as JSON gives them back
    assert got == want


def test_record_covers_the_cases_the_families_ship():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(CASES)
    assert [want[c]["kept_tensors"] for c in ("pointnet", "pointnet_noft", "pointnet2", "pointconv", "dgcnn")] == [47, 32, 56, 47, 17]
    # the per-family "also as three bf16 terms" rules: DGCNN's heads carry none, only conv5_bf3
    d = want["dgcnn"]["struct"]
    assert all(d[n]["w_bf3"] is None for n in ("conv5", "fc1", "fc2", "fc3")) and d["conv5_bf3"]["dtype"] == "torch.int16"
