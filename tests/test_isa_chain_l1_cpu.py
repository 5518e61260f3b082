"""CPU: layer 1 of the PointNet chain kernel's bf16x3 instantiations left the fp32 matrix instruction.

In the libiq_hip.so that ships, every pn_chain_kernel<*, 3, *> (feature STN, trunk, their 64-row twins, trunk with arg-max) holds
no v_mfma_f32_32x32x2_f32 any more - layers 1 to 3 all run as six bf16 products on v_mfma_f32_16x16x32_bf16 - and
every pn_chain_kernel<*, 2, *> (pre-pool, the fp32 twins) still holds it.  Registers, scratch and LDS of the bf16x3 kernels are
bounded by tests/test_isa_chain_shape_cpu.py."""
import os
import re
import sys

import pytest

from interpret_quality_amd import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_audit  # noqa: E402

FP32_MFMA = "v_mfma_f32_32x32x2_f32"


@pytest.fixture(scope="module")
def chain():
    """{(mode, L3V, ARGMAX) as written in the demangled name: {mfma instruction: count}} of every pn_chain_kernel"""
    if not os.path.exists(os.path.join(isa_audit.LLVM_BIN, "llvm-objdump")):
        pytest.skip("llvm-objdump not found")
    audit = isa_audit.audit(build.build(verbose=False))
    out = {}
    for sym, name in isa_audit.demangle(sorted(audit)).items():
        m = re.search(r"\bpn_chain_kernel<([^()]*)>\(", name)
        if m:
            out[tuple(a.strip() for a in m.group(1).split(","))] = audit[sym]["mfma_kinds"]
    return out


def test_bf16x3_chain_kernels_hold_no_fp32_mfma(chain):
    bf3 = {k: v for k, v in chain.items() if k[1] == "3"}
    assert len(bf3) == 5, sorted(chain)          # feature STN, trunk, their two 64-row twins, trunk with arg-max
    for k, kinds in bf3.items():
        assert FP32_MFMA not in kinds, (k, kinds)
        assert set(kinds) == {"v_mfma_f32_16x16x32_bf16"}, (k, kinds)


def test_fp32_chain_kernels_still_hold_it(chain):
    fp32 = {k: v for k, v in chain.items() if k[1] == "2"}
    assert len(fp32) >= 3, sorted(chain)         # pre-pool, feature STN twin, trunk twin (and the trunk's arg-max twin)
    for k, kinds in fp32.items():
        assert kinds.get(FP32_MFMA, 0) >= 256, (k, kinds)
