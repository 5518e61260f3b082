"""The PointNet step on distinct coalitions, without a GPU: the diagnostic entry for the slot map is declared, bound and versioned;
the workspace grew by no more than 16 bytes per coalition for the slot map; the copy kernel of the former scheme is gone from the
sources and the heads hand the device's row count to the dense launcher."""
import os
import re

from conftest import REPO
from interpret_quality_amd import _lib

CSRC = os.path.join(REPO, "interpret_quality_amd", "csrc")


def test_slot_entry_is_declared_bound_and_versioned():
    header = open(os.path.join(REPO, "include", "iq_debug.h")).read()
    declared = set(re.findall(r"\b(iq_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in ("iq_debug_pointnet_slots", "iq_debug_pointnet_reps"):
        assert name in declared and name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["iq_debug_pointnet_slots"] == _lib.SIGNATURES["iq_debug_pointnet_reps"]
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", open(os.path.join(REPO, "include", "iq.h")).read()).group(1))
    assert _lib.ABI_VERSION == _lib.load().iq_version() == version >= 119


def test_workspace_grows_by_at_most_16_bytes_per_coalition():
    """Per coalition the step held, before the slot map: a row list of kRowCap = 4096 + 64 uint16, nrows / order / bin_of (int32),
    gbuf (1024), h1 (512), h2 (256), trans (9) and tfp (4096) floats.  Every array is rounded up to 256 bytes once, whatever B."""
    before = 2 * (4096 + 64) + 3 * 4 + 4 * (1024 + 512 + 256 + 9 + 4096)
    lib = _lib.load()
    for sizes in (lib.iq_pointnet_workspace_bytes, lib.iq_pointnet_wide_workspace_bytes):
        for nc, n, r in ((1, 1024, 32), (3, 200, 8)):
            small, large = sizes(64, nc, n, r), sizes(64 + 33000, nc, n, r)
            per_item = (large - small) / 33000.0
            assert before < per_item <= before + 16 + 12 * 256 / 33000.0, (per_item, before)


def test_one_path_for_every_item():
    src = open(os.path.join(CSRC, "iq_pointnet.hip")).read() + open(os.path.join(CSRC, "iq_pointnet_chain.h")).read()
    assert "pn_dup_copy_kernel" not in src and "dup_rep" not in src
    body = src[src.index("int pointnet_coalitions("):src.index('extern "C" int iq_pointnet_coalitions_crt')]
    heads = re.findall(r"launch_linear\((ws\.[^;]*?, true)\)", body)
    assert len(heads) == 10                                    # nine layers; the last one once by slot, once in place
    assert sum("n_dev, nullptr, 0, true" in h for h in heads) == 9
    assert body.index("launch_compact(") < body.index("pn_rows_kernel,")
