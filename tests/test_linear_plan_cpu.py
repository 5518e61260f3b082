"""CPU: the dense layer's dispatch (csrc/iq_linear_plan.h - which kernel, rows, columns and grid every launch of
launch_linear / launch_linear_splitk / launch_linear_pool gets) enumerated by a stand-alone program over the product's layers,
CU counts 1 .. 304, every flag and twin the dispatch reads and row counts around every edge of the round rule.
tests/cpp/linear_plan_check.cpp names the invariants; it is compiled with the address and undefined-behaviour sanitizers and run
as a plain child process."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "interpret_quality_amd", "csrc")


def test_every_plan_of_the_dense_dispatch_holds_its_invariants(tmp_path):
    exe = str(tmp_path / "linear_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "linear_plan_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    checked = re.search(r"(\d+) plans checked", run.stdout)
    assert checked and int(checked.group(1)) > 0, run.stdout


def test_the_plan_header_is_host_only_and_the_launchers_hold_no_dispatch():
    """iq_linear_plan.h includes nothing but iq_twin.h (so no HIP header, no runtime call), and the pointer side of the dispatch
    in iq_linear.hip names every dense-layer kernel in one switch: no launcher tests M, the layer's sizes or a twin itself."""
    header = open(os.path.join(CSRC, "iq_linear_plan.h")).read()
    assert re.findall(r'#include\s+(\S+)', header) == ['"iq_twin.h"']
    src = open(os.path.join(CSRC, "iq_linear.hip")).read()
    host = src[src.index("int run_segment("):src.index('extern "C" int iq_linear(')]
    assert host.count("switch (s.kernel)") == 1
    for kernel in ("pn_gemm_bf3_kernel", "pn_gemm_bf3_short_kernel", "pn_gemm_lds_kernel", "pn_linear_kernel"):
        assert kernel not in host[host.index("int run_plan("):], kernel
    assert "iq::twin() ==" not in host and "iq::twin() !=" not in host and "cout % 256" not in host
