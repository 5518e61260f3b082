"""CPU: the bf16x3 instantiations of the PointNet chain kernel in the libiq_hip.so that ships run on v_mfma_f32_16x16x32_bf16.

The chain kernel is power-bound and the 16x16x32 shape draws less power per FLOP than 32x32x16 (DESIGN.md 5a,
profiles/chain_shape_probe.txt, profiles/chain_shape_ab.txt), so every pn_chain_kernel<*, 3, *> holds the one instruction and not
the other; and the register budget the shape was fitted into is kept: no scratch (so no spill), at most 256 registers per lane
(AGPRs included) and an LDS size that leaves two workgroups per CU (160 KiB).  The grouped and GEMM bf16x3 kernels stay on
32x32x16 (tests/test_isa_cpu.py looks for them)."""
import os
import re
import sys

import pytest

from interpret_quality_amd import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_audit  # noqa: E402


@pytest.fixture(scope="module")
def chain():
    """{demangled name: (instruction audit, resources)} of every pn_chain_kernel<*, 3, *> in the shipped library"""
    if not os.path.exists(os.path.join(isa_audit.LLVM_BIN, "llvm-objdump")):
        pytest.skip("llvm-objdump not found")
    so = build.build(verbose=False)
    audit, res = isa_audit.audit(so), isa_audit.resources(so)
    out = {}
    for sym, name in isa_audit.demangle(sorted(audit)).items():
        m = re.search(r"\bpn_chain_kernel<([^()]*)>\(", name)
        if m and [a.strip() for a in m.group(1).split(",")][1] == "3":
            assert sym in res, "no code-object metadata for %s" % name
            out[name] = (audit[sym], res[sym])
    return out


def test_bf16x3_chain_kernels_use_the_16x16x32_shape_only(chain):
    assert len(chain) >= 3, sorted(chain)            # feature-STN, trunk, trunk with arg-max
    for name, (a, _) in chain.items():
        assert a["mfma_kinds"].get("v_mfma_f32_16x16x32_bf16", 0) >= 96, (name, a["mfma_kinds"])
        assert "v_mfma_f32_32x32x16_bf16" not in a["mfma_kinds"], (name, a["mfma_kinds"])


def test_bf16x3_chain_kernels_keep_their_register_and_lds_budget(chain):
    for name, (_, r) in chain.items():
        assert r["scratch"] == 0 and not r.get("dynamic_stack", False), (name, r)
        assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 256, (name, r)
        assert 2 * r["lds"] <= 160 * 1024, (name, r)
