"""The experiment knobs of libiq_hip.so (iq_set_tuning, include/iq_debug.h) by name, for tests, bench tools and A/B runs.

A twin is a reference form of a product kernel (csrc/iq_twin.h lists them once; TWINS mirrors that list and
tests/test_cabi_cpu.py holds the two together).  A knob is state of the calling thread and applies to every later launch of
that thread, so it is only ever selected through a context manager that checks the library's answer - a refused pair raises
IqError instead of leaving the thread on the product path - and sets the knob back to 0 on the way out.  Selections of one key
do not nest (the inner exit would clear the outer one):

    with tuning.twin("chain_l3_fp32"):
        ref = run()
    ref = tuning.tuned("chain_l3_fp32", run)        # the same
"""
import contextlib
import threading

from . import _lib

KEY_NO_LDS_GEMM, KEY_TWIN = 3, 5

# name (the enumerator kTwin<Name> of csrc/iq_twin.h in snake case) -> key-5 value
TWINS = {
    "edge_gemm_l2": 7,
    "edge_gemm_lds": 8,
    "knn_compact": 12,
    "pc_knn": 14,
    "pc_grouped_mlp": 15,
    "knn_fp32_rank": 20,
    "pn2_member_walk": 21,
    "knn_fp32_mfma": 22,
    "pc_two_kernel": 31,
    "chain_l3_fp32": 54,
    "chain_l3_fp32_no_tail16": 55,
    "group_fp32": 56,
    "dense_fp32": 57,
    "chain_l3_single": 58,
    "dense_tile128": 59,
    "chain_no_dedup": 60,
    "group_fp32_chunk64": 64,
}

_active = threading.local()     # the knobs are per thread in the library, so is the record of what this module has set


def value_of(which):
    """The key-5 value of `which`: a name or a value of TWINS, or 0 / None for the product path.  Anything else raises."""
    if which is None:
        return 0
    if isinstance(which, str):
        if which not in TWINS:
            raise KeyError("unknown twin %r (interpret_quality_amd.tuning.TWINS)" % (which,))
        return TWINS[which]
    if type(which) is not int or (which != 0 and which not in TWINS.values()):
        raise ValueError("%r is not the value of a twin (interpret_quality_amd.tuning.TWINS)" % (which,))
    return which


@contextlib.contextmanager
def _knob(key, value):
    active = _active.__dict__.setdefault("knobs", {})
    if key in active:       # also for value 0: inside a selection the product path is not what would run
        raise RuntimeError("iq_set_tuning(%d, %d) is still selected on this thread; selections of a key do not nest" % (key, active[key]))
    if not value:
        yield
        return
    lib = _lib.load()
    _lib.check(lib.iq_set_tuning(key, value), "iq_set_tuning(%d, %d)" % (key, value))
    active[key] = value
    try:
        yield
    finally:
        del active[key]
        _lib.check(lib.iq_set_tuning(key, 0), "iq_set_tuning(%d, 0)" % key)


def twin(which):
    """Context manager: the calling thread's launches take the twin `which` (value_of) inside, the product paths after."""
    return _knob(KEY_TWIN, value_of(which))


def tuned(which, fn):
    """fn() under twin(which)."""
    with twin(which):
        return fn()


def no_lds_gemm():
    """Context manager: dense layers without the LDS-staged GEMM (key 3) inside."""
    return _knob(KEY_NO_LDS_GEMM, 1)
