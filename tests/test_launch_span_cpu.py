"""CPU: what tests/test_launch_span_gpu.py relies on.  The table of capped routes is complete, every entry really crosses the
boundaries it names (from the size functions of the built library) and is the GPU file's parameter list; ``rows_differ`` sees
the three shapes a narrow index leaves behind; and no size, count or offset crosses the C ABI through a narrower ctypes type than
the header declares (a ``*_workspace_bytes`` bound as c_int would truncate 36 GiB without a word)."""
import ast
import ctypes
import importlib
import inspect
import os
import pkgutil
import re

import numpy as np
import pytest

import launch_span as L
from interpret_quality_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def routes():
    build.build(verbose=False)  # hipcc cross-compiles gfx950 without a GPU
    return L.routes()


# ---- the table -------------------------------------------------------------------------------------------------------------

def capped_classes():
    """Every class of the package that carries a ``max_clouds_per_call`` and can be instantiated as a model (a name without a
    leading underscore, defined in the module it is found in)."""
    import interpret_quality_amd
    out = set()
    for info in pkgutil.iter_modules(interpret_quality_amd.__path__):
        mod = importlib.import_module("interpret_quality_amd." + info.name)
        for name, cls in inspect.getmembers(mod, inspect.isclass):
            if cls.__module__ == mod.__name__ and not name.startswith("_") and hasattr(cls, "max_clouds_per_call"):
                out.add(cls)
    return out


def test_every_class_with_a_launch_cap_is_in_the_table(routes):
    found = capped_classes()
    assert len(found) >= 4
    assert found == {L.model_class(f) for f in L.FAMILIES} == {L.model_class(r.family) for r in routes}
    for family in L.FAMILIES:
        mine = {(r.route, r.twin) for r in routes if r.family == family}
        want = {"forward_points", "coalition_logits", "coalition_logits_wide", "compact"}
        assert want | ({"coalition_logits_cached"} if family == "pointconv" else set()) == {r for r, _ in mine}, family
    # one twin per kernel body that tests/test_f64_families_gpu.py::TWINS lists for a route (its table has no dgcnn row: gcnn's
    # EdgeConv twins are DGCNN's kernels); every named twin exists and belongs to the family it is listed under
    from interpret_quality_amd import tuning
    listed = {(r.family, r.twin) for r in routes if r.twin}
    assert {t for _, t in listed} == {"group_fp32", "pn2_member_walk", "pc_two_kernel", "edge_gemm_l2", "edge_gemm_lds"} <= set(tuning.TWINS)
    text = open(os.path.join(REPO, "tests", "test_f64_families_gpu.py")).read()
    twins = ast.literal_eval(re.search(r"^TWINS = (\{.*?\})$", text, flags=re.M | re.S).group(1))
    for family, twin in listed:
        assert twin in twins["gcnn" if family == "dgcnn" else family], (family, twin)


def test_every_route_crosses_the_boundaries_it_names_at_its_cap(routes):
    lib = _lib.load()
    assert list(L.SPANS.values()) == [1 << 31, 1 << 32, 1 << 33]
    for r in routes:
        assert r.cap == L.model_class(r.family).max_clouds_per_call
        # straight from the library, beside the engine class's formula routes() went through
        if r.family == "pointnet2":
            want = lib.iq_pointnet2_coalitions_workspace_bytes(r.cap, r.nc, r.n) if r.nc else lib.iq_pointnet2_workspace_bytes(r.cap)
        elif r.family == "pointconv":
            want = lib.iq_pointconv_coalitions_workspace_bytes(r.cap, r.nc, r.n) if r.nc else lib.iq_pointconv_workspace_bytes(r.cap, r.n)
        else:
            want = lib.iq_dgcnn_workspace_bytes(r.cap, r.n)
        assert r.workspace_bytes == want > 1 << 32, r
        assert "4GiB" in r.crosses and r.crosses == tuple(k for k, v in L.SPANS.items() if want > v), r
        # the cloud is the smallest the family takes at which a coalition's share is still whole, and a game of R regions has R points
        assert r.n >= r.regions or r.regions <= 64
        need = L.size_fn(r.family, r.route)
        per = lambda n: (need(r.cap, n) - need(r.cap // 2, n)) / (r.cap - r.cap // 2)
        assert per(r.n) >= L.FULL_SIZE * per(L.MAX_POINTS), r
        # a share, not the head of the workspace: the last coalition of the launch starts behind 4 GiB
        assert (r.cap - 1) * per(r.n) > 1 << 32, r
    sizes = {(r.family, r.route): r.n for r in routes}
    assert sizes[("pointconv", "forward_points")] == 64 and sizes[("pointnet2", "forward_points")] == 128
    assert {sizes[(f, rt)] for f in ("dgcnn", "gcnn") for rt in ("forward_points", "coalition_logits", "compact")} == {1024}


def test_the_gpu_file_runs_exactly_the_table(routes):
    import test_launch_span_gpu as G
    ids = [r.id for r in routes]
    assert len(set(ids)) == len(ids) == len(L.TABLE)
    assert G.CASES == ids, "tests/test_launch_span_gpu.py::CASES is stale: %s" % sorted(set(G.CASES) ^ set(ids))
    fn = G.test_every_row_of_a_launch_at_the_cap_equals_the_same_row_from_small_launches
    marks = [m for m in fn.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and list(marks[0].args[1]) == ids
    assert G.pytestmark.name == "gpu"


# ---- the comparison --------------------------------------------------------------------------------------------------------

def reference_rows(b=4096, c=10):
    return np.random.default_rng(0).standard_normal((b, c)).astype(np.float32)


def test_rows_differ_returns_nothing_for_an_exact_copy():
    import torch
    ref = reference_rows()
    ref[5, 3] = np.nan                       # bits are compared: a NaN equals itself
    ref[6, 0], ref[7, 0] = 0.0, -0.0
    assert L.rows_differ(ref.copy(), ref) == [] and repr(L.rows_differ(ref.copy(), ref)) == "[]"
    assert L.rows_differ(torch.from_numpy(ref.copy()), torch.from_numpy(ref), 9e6) == []
    signed = ref.copy()
    signed[6, 0], signed[7, 0] = -0.0, 0.0   # equal as numbers, not as bits
    assert L.rows_differ(signed, ref) == [6, 7]
    with pytest.raises(AssertionError):
        L.rows_differ(ref[:100], ref)


def test_rows_differ_sees_rows_past_a_position_all_zero():
    """A buffer load past num_records returns 0: with 9.26 MB per coalition (PointConv) the rows from position 232 on."""
    ref = reference_rows()
    per = 38858232576 / 4096
    k = int((1 << 31) // per) + 1
    big = ref.copy()
    big[k:] = 0
    bad = L.rows_differ(big, ref, per)
    assert bad == list(range(k, 4096))
    assert "first at position %d " % k in bad.message and "behind the 2GiB boundary" in bad.message and "is all zero" in bad.message
    assert ("byte offset %d " % int(k * per)) in bad.message and repr(bad) == bad.message


def test_rows_differ_sees_a_row_that_is_a_copy_of_an_earlier_row():
    """A wrapped 32-bit offset: position i reads what belongs to position i - k, k = 4 GiB / bytes per coalition."""
    ref = reference_rows()
    per = 18668912896 / 4096                  # DGCNN at N = 1024
    k = int((1 << 32) // per) + 1
    big = ref.copy()
    big[k:] = ref[:-k]
    bad = L.rows_differ(big, ref, per)
    assert bad == list(range(k, 4096))
    assert "first at position %d " % k in bad.message and "behind the 4GiB boundary" in bad.message
    assert "holds the reference row of position 0 (%d rows earlier)" % k in bad.message


def test_rows_differ_sees_one_late_row_off_by_one_ulp_in_one_logit():
    ref = reference_rows()
    per = 12671041536 / 4096                  # PointNet++
    big = ref.copy()
    big[4001, 7] = np.nextafter(big[4001, 7], np.float32(np.inf))
    bad = L.rows_differ(big, ref, per)
    assert bad == [4001]
    assert "1 of 4096 rows differ" in bad.message and "behind the 8GiB boundary" in bad.message
    assert "differs in 1 of 10 logits, first at logit 7" in bad.message
    early = ref.copy()
    early[3, 0] = np.nextafter(early[3, 0], np.float32(-np.inf))
    assert "below every boundary" in L.rows_differ(early, ref, per).message


# ---- ABI widths ------------------------------------------------------------------------------------------------------------

C_KINDS = {"int": "int32", "int32_t": "int32", "size_t": "int64", "uint64_t": "int64", "int64_t": "int64", "double": "double",
           "float": "float", "void": "void"}


def c_kind(text):
    """A C parameter or return type (comments gone, the parameter's name still on it or not) -> pointer / int32 / int64 / double
    / float / void; anything else is returned as it stands and matches nothing."""
    text = " ".join(re.sub(r"\bconst\b", " ", text).split())
    if "*" in text or "[" in text or text.split()[0] == "iq_stream_t":      # iq_stream_t is a void*
        return "pointer"
    words = text.split()
    for take in (len(words), len(words) - 1):            # with or without a trailing parameter name
        if " ".join(words[:take]) in C_KINDS:
            return C_KINDS[" ".join(words[:take])]
    return text


def ctypes_kind(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    if t in (ctypes.c_double, ctypes.c_float):
        return {ctypes.c_double: "double", ctypes.c_float: "float"}[t]
    if issubclass(t, ctypes._SimpleCData) and t._type_ in "iIlLqQ":
        if t is ctypes.c_int:                                                # a C int, signed
            return "int32"
        if ctypes.sizeof(t) == 8:
            return "int64"
    return repr(t)


def header_text(name):
    """The header as tests/test_cabi_cpu.py reads it: block comments dropped."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def prototypes():
    """{name: (return type, [parameter types])} of every function declared in include/iq.h and include/iq_debug.h."""
    out = {}
    for h in ("iq.h", "iq_debug.h"):
        text = re.sub(r"//[^\n]*", "", header_text(h))
        text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)                 # preprocessor lines (none is continued)
        text = text.replace('extern "C" {', "")
        while re.search(r"\{[^{}]*\}", text):                               # struct bodies
            text = re.sub(r"\{[^{}]*\}", "", text)
        for stmt in text.split(";"):
            m = re.match(r"\s*([\w\s\*]+?)\s*\b(iq_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
            if not m:
                continue
            ret, name, params = m.groups()
            assert name not in out, name
            params = [p.strip() for p in params.split(",")]
            out[name] = (ret, [] if params == ["void"] else params)
    return out


def test_no_argument_crosses_the_c_abi_narrower_than_the_header_declares():
    declared = set()
    for h in ("iq.h", "iq_debug.h"):
        assert "\\\n" not in header_text(h)
        declared |= set(re.findall(r"\b(iq_[a-z0-9_]+)\s*\(", header_text(h)))      # the regex of tests/test_cabi_cpu.py
    protos = prototypes()
    assert set(protos) == declared == set(_lib.SIGNATURES), set(protos) ^ declared | declared ^ set(_lib.SIGNATURES)
    assert len(protos) >= 108
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        res, args = _lib.SIGNATURES[name]
        if c_kind(ret) != ctypes_kind(res):
            bad.append("%s returns %r, bound as %r" % (name, ret, res))
        if len(params) != len(args):
            bad.append("%s takes %d arguments, bound with %d" % (name, len(params), len(args)))
            continue
        for i, (p, a) in enumerate(zip(params, args)):
            assert c_kind(p) in ("pointer", "int32", "int64", "double", "float"), (name, i, p)
            if c_kind(p) != ctypes_kind(a):
                bad.append("%s argument %d is %r, bound as %r" % (name, i, p, a))
    assert not bad, "\n".join(bad)
    # what the launches at the cap depend on, by name: sizes come back and go in as 64-bit values
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.endswith("_bytes") or "_bytes_" in name:
            assert ctypes_kind(res) == "int64", name
    for name in ("iq_pointconv_forward", "iq_pointconv_coalitions_cached", "iq_pointnet2_coalitions", "iq_dgcnn_coalitions_wide"):
        assert [p for p in protos[name][1] if "workspace_bytes" in p or "ws_bytes" in p], (name, protos[name][1])


def test_the_type_classifiers_tell_a_narrow_binding_from_a_wide_one():
    assert c_kind("size_t workspace_bytes") == "int64" != ctypes_kind(ctypes.c_int)
    assert c_kind("size_t") == ctypes_kind(ctypes.c_size_t) == ctypes_kind(ctypes.c_uint64) == ctypes_kind(ctypes.c_int64) == "int64"
    assert c_kind("int B") == c_kind("int32_t x") == ctypes_kind(ctypes.c_int) == ctypes_kind(ctypes.c_int32) == "int32"
    assert ctypes_kind(ctypes.c_uint32) not in ("int32", "int64") and ctypes_kind(ctypes.c_long) == "int64"
    assert c_kind("const float* clouds") == c_kind("iq_stream_t stream") == c_kind("const char*") == "pointer"
    assert ctypes_kind(ctypes.POINTER(ctypes.c_double)) == ctypes_kind(ctypes.c_char_p) == "pointer"
    assert c_kind("double bandwidth") == ctypes_kind(ctypes.c_double) == "double" != ctypes_kind(ctypes.c_float) == c_kind("float radius")
    assert c_kind("unsigned long n") not in ("pointer", "int32", "int64", "double", "float")
