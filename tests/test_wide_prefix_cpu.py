"""CPU: the surface of the prefix route of wide games - iq_pointnet_prefix_coalitions_wide is declared, exported, bound with the
header's argument count and versioned; final_wide_shapley.py has --route; wide.shapley refuses an unknown route before any device
work.  What the entry computes: tests/test_wide_prefix_gpu.py."""
import os
import re
import subprocess
import sys

import pytest

from interpret_quality_amd import _lib, build, wide, wide_stage

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "iq_pointnet_prefix_coalitions_wide"


def _header():
    return open(os.path.join(REPO, "include", "iq.h")).read()


def _declaration():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % ENTRY, code)
    assert m, "%s is not declared in include/iq.h" % ENTRY
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_point():
    params = _declaration()
    assert len(params) == 15
    assert params[0].startswith("const iq_pointnet_weights*") and params[-1] == "iq_stream_t stream"
    assert [p.split()[-1] for p in params[4:6]] == ["orders", "cloud_of"] and all(p.startswith("const int32_t*") for p in params[4:6])
    assert [p for p in params if p.startswith("int ")] == ["int S", "int nclouds", "int N", "int R"]


def test_library_exports_the_entry_point_and_the_binding_has_the_headers_argument_count():
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, ENTRY) and ENTRY in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[ENTRY]
    assert len(args) == len(_declaration()) and len(getattr(lib, ENTRY).argtypes) == len(args)


def test_abi_version_is_at_least_107_on_all_three_sides():
    build.build(verbose=False)
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", _header()).group(1))
    assert _lib.ABI_VERSION == _lib.load().iq_version() == version >= 107


def test_final_wide_shapley_help_lists_route():
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "final_wide_shapley.py"), "--help"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--route" in r.stdout and "prefix" in r.stdout and "keep" in r.stdout
    assert wide_stage.make_args(["--model", "pointnet"]).route is None
    assert wide_stage.make_args(["--model", "pointnet", "--route", "keep"]).route == "keep"
    with pytest.raises(SystemExit):
        wide_stage.make_args(["--model", "pointnet", "--route", "nonsense"])


def test_shapley_refuses_an_unknown_route_before_touching_a_device():
    with pytest.raises(_lib.IqError, match="route"):
        wide.shapley(None, None, None, None, None, None, route="nonsense")      # nothing else is looked at first
    assert wide.ROUTES == ("prefix", "keep") and wide.DEFAULT_ROUTE in wide.ROUTES
