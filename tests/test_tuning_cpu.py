"""CPU: the selector of experiment twins (interpret_quality_amd/tuning.py).  What it sends to iq_set_tuning is recorded by a
stand-in for the loaded library; the last test goes to the real one (iq_set_tuning is host-only).  That the names are the list
of csrc/iq_twin.h is test_cabi_cpu.py's test_set_tuning_accepts_the_twins_and_refuses_the_rest."""
import threading

import pytest

from interpret_quality_amd import _lib, build, tuning


class Recorder:
    """Stands in for the ctypes library: records every (key, value), refuses the pairs in `refuse` with IQ_EINVAL."""

    def __init__(self, refuse=()):
        self.calls, self.refuse = [], set(refuse)

    def iq_set_tuning(self, key, value):
        self.calls.append((key, value))
        return -1 if (key, value) in self.refuse else 0

    def iq_last_error(self):
        return b"iq_set_tuning: key %d value %d is not an experiment knob" % self.calls[-1]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


def test_twin_sets_the_knob_on_entry_and_clears_it_on_exit(rec):
    with tuning.twin("chain_l3_fp32"):
        assert rec.calls == [(5, 54)]
    assert rec.calls == [(5, 54), (5, 0)]
    with tuning.twin(tuning.TWINS["chain_l3_single"]):      # by value; and the thread accepts a selection again
        assert rec.calls[2:] == [(5, 58)]
    assert rec.calls[2:] == [(5, 58), (5, 0)]
    assert tuning.tuned("dense_fp32", lambda: list(rec.calls[4:])) == [(5, 57)]
    with tuning.no_lds_gemm():
        assert rec.calls[6:] == [(3, 1)]
    assert rec.calls[4:] == [(5, 57), (5, 0), (3, 1), (3, 0)]


def test_twin_clears_the_knob_when_the_body_raises(rec):
    with pytest.raises(ZeroDivisionError):
        with tuning.twin("chain_l3_fp32"):
            1 / 0
    assert rec.calls == [(5, 54), (5, 0)]
    with pytest.raises(ZeroDivisionError):
        tuning.tuned("group_fp32", lambda: 1 / 0)
    assert rec.calls[2:] == [(5, 56), (5, 0)]


@pytest.mark.parametrize("which", [0, None])
def test_the_product_path_sets_nothing(rec, which):
    with tuning.twin(which):
        pass
    assert tuning.tuned(which, lambda: 3) == 3
    assert rec.calls == []


def test_a_refused_pair_raises(rec):
    rec.refuse.add((5, 54))
    with pytest.raises(_lib.IqError, match="key 5 value 54"):
        with tuning.twin("chain_l3_fp32"):
            pytest.fail("the body ran on the product path")
    assert rec.calls == [(5, 54)]
    with tuning.twin("chain_l3_single"):                    # the failed selection left nothing active
        pass
    rec.refuse.add((5, 0))                                   # a refused restore is not silent either
    with pytest.raises(_lib.IqError, match="key 5 value 0"):
        with tuning.twin("chain_l3_single"):
            pass


@pytest.mark.parametrize("which", ["chain_l3", "54", "", 53, 91, -1, 5.0, True, (5, 54)], ids=repr)
def test_an_unknown_name_or_value_raises_before_the_library_is_called(rec, which):
    with pytest.raises((KeyError, ValueError)):
        tuning.twin(which)
    with pytest.raises((KeyError, ValueError)):
        tuning.tuned(which, lambda: pytest.fail("the body ran"))
    assert rec.calls == []


def test_nesting_raises(rec):
    with tuning.twin("chain_l3_fp32"):
        with pytest.raises(RuntimeError, match="do not nest"):
            with tuning.twin("chain_l3_single"):
                pytest.fail("the body ran")
        with pytest.raises(RuntimeError, match="do not nest"):
            with tuning.twin(0):                             # not the product path in here either
                pytest.fail("the body ran")
        with tuning.no_lds_gemm():                           # another key: the two combine
            with pytest.raises(RuntimeError, match="do not nest"):
                with tuning.no_lds_gemm():
                    pytest.fail("the body ran")
        other = []                                           # the knobs are per thread: another thread is free
        t = threading.Thread(target=lambda: other.append(tuning.tuned("dense_fp32", lambda: 1)))
        t.start()
        t.join()
        assert other == [1]
    assert rec.calls == [(5, 54), (3, 1), (3, 0), (5, 57), (5, 0), (5, 0)]


def test_tuned_against_the_library():
    build.build(verbose=False)
    lib = _lib.load()
    assert tuning.tuned("chain_no_dedup", lambda: "value") == "value"
    for name in tuning.TWINS:                                # every name is accepted, and each exit leaves the thread free
        with tuning.twin(name):
            pass
    with tuning.no_lds_gemm():
        pass
    assert lib.iq_set_tuning(5, 91) == -1 and lib.iq_set_tuning(5, 0) == 0
