"""CPU: the counter-based draw of a wide game's rows - the NumPy restatement of the contract (tests/kshap_counter_ref.py) against
Philox4x32-10's known answers, the size law and the uniform law of the subsets, the layout of the rows, the independence of a range
from the rows around it, and the estimator's error on such rows against the stream draw's; the plumbing (ABI 116) and the refusals
that need no device."""
import os
import re
from itertools import combinations

import numpy as np
import pytest

import exact_ref
import kernelshap_ref as narrow
import kshap_counter_ref as ref
from interpret_quality_amd import _lib, build, hip_ops, wide_kernelshap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 99.9 % points of the chi-square law (standard tables), by degrees of freedom
CHI2_999 = {4: 18.467, 5: 20.515, 14: 36.123, 19: 43.820}


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox4x32_10_known_answers():
    for counter, key, want in (([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                               ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                               ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
                                "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert _hex(ref.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))) == want
    # vectorised: the three blocks in one call, and a key that carries bits above 32 is masked
    c = np.array([[0] * 4, [0xFFFFFFFF] * 4], dtype=np.uint64)
    k = np.array([[0] * 2, [0xFFFFFFFF] * 2], dtype=np.uint64)
    out = ref.philox4x32_10(c, k)
    assert _hex(out[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and _hex(out[1]) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert np.array_equal(ref.sizes((1 << 32) + 1, (7 << 32) + 2, 0, 50, 65), ref.sizes(1, 2, 0, 50, 65))


def test_sizes_follow_the_size_law_and_subsets_of_a_size_are_uniform():
    """60 000 samples at R = 6, seed 1, stream 0 (fixed: deterministic).  The size histogram against size_cdf's law and, per size,
    the histogram of the subsets against the uniform law: every subset occurs and each chi-square statistic is below the 99.9 %
    point of its degrees of freedom.  The restatement gives 6.5 on 4 degrees of freedom for the sizes and 4.2 / 10.4 / 13.7 / 8.6 /
    4.3 on 5 / 14 / 19 / 14 / 5 for the subsets."""
    r, count = 6, 60000
    rows, sizes = ref.rows(1, 0, 0, count, r, paired=False)
    assert rows.shape == (count, 1) and sizes.min() == 1 and sizes.max() == r - 1
    p = np.diff(np.concatenate([[0.0], wide_kernelshap.size_cdf(r)]))
    seen = np.bincount(sizes, minlength=r)[1:]
    stat = float(((seen - count * p) ** 2 / (count * p)).sum())
    print("sizes: chi-square %.1f on %d degrees of freedom" % (stat, r - 2))
    assert stat < CHI2_999[r - 2]
    masks = rows[:, 0].astype(np.int64)
    assert np.array_equal(np.array([bin(int(x)).count("1") for x in masks]), sizes)
    for s in range(1, r):
        subsets = [sum(1 << i for i in c) for c in combinations(range(r), s)]
        mine = masks[sizes == s]
        hist = np.array([(mine == x).sum() for x in subsets])
        assert hist.sum() == len(mine) and hist.min() > 0, "a subset of size %d never occurs" % s
        expect = len(mine) / len(subsets)
        stat = float(((hist - expect) ** 2 / expect).sum())
        print("size %d: chi-square %.1f on %d degrees of freedom" % (s, stat, len(subsets) - 1))
        assert stat < CHI2_999[len(subsets) - 1]


@pytest.mark.parametrize("r", [2, 6, 64, 65, 1023, 1024])
def test_rows_have_the_layout_of_the_contract(r):
    count, w = 40, (r + 63) // 64
    rows, sizes = ref.rows(3, 5, 0, count, r)
    assert rows.shape == (2 * count, w) and rows.dtype == np.uint64 and sizes.dtype == np.int32
    full = hip_ops.region_words(np.arange(r), r)
    assert np.array_equal(rows[0::2] ^ rows[1::2], np.broadcast_to(full, (count, w))) and not np.any(rows[0::2] & rows[1::2])
    if r & 63:
        assert not np.any(rows[:, -1] >> np.uint64(r & 63)), "a bit at or above R"
    pop = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1).sum(axis=1)
    assert np.array_equal(pop[0::2], sizes) and np.array_equal(pop[1::2], r - sizes)
    single, sizes1 = ref.rows(3, 5, 0, count, r, paired=False)
    assert np.array_equal(single, rows[0::2]) and np.array_equal(sizes1, sizes)
    other, _ = ref.rows(3, 6, 0, count, r)
    assert r == 2 or not np.array_equal(other, rows)                   # another stream, other rows
    if r > 2:
        assert not np.array_equal(ref.rows(4, 5, 0, count, r)[0], rows)


def test_a_range_drawn_alone_is_that_range_of_a_longer_draw():
    for r in (6, 65, 1024):
        long_rows, long_sizes = ref.rows(1, 2, 0, 300, r)
        for lo, n in ((0, 1), (1, 257), (258, 42)):
            part, sizes = ref.rows(1, 2, lo, n, r)
            assert np.array_equal(part, long_rows[2 * lo:2 * (lo + n)]) and np.array_equal(sizes, long_sizes[lo:lo + n])
    # a first whose low word wraps: samples 2^32 - 2 .. 2^32 + 1
    first = (1 << 32) - 2
    four, sizes = ref.rows(1, 0, first, 4, 65)
    for j in range(4):
        one, s1 = ref.rows(1, 0, first + j, 1, 65)
        assert np.array_equal(one, four[2 * j:2 * j + 2]) and s1[0] == sizes[j]
    lo, hi = ref._index_words(first, 4)
    assert lo.tolist() == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1] and hi.tolist() == [0, 0, 1, 1]
    assert not np.array_equal(four[4:6], ref.rows(1, 0, 0, 1, 65)[0])     # m = 2^32 is not m = 0: the high word enters


def test_estimator_on_counter_rows_is_as_good_as_on_stream_rows():
    """R = 10, a fixed random value table, exact values by enumeration (tests/exact_ref.py), the closed form with the analytic
    Gram matrix (tests/kernelshap_ref.py).  RMS error over seeds 1 .. 20 at 2000 paired rows, counter rows against rows of the
    stream draw (``host_draw`` + ``rows_from_orders``).  Measured with the restatement: ratio 1.0232 for these seeds (RMS errors
    0.04854 and 0.04744); over ten disjoint sets of 20 seeds the ratio has mean 1.005 and standard deviation 0.0858.  The band
    is the measured ratio +- three times that spread, 1.0232 +- 0.2575: a draw with the wrong size law or a biased subset
    moves the ratio."""
    n = 10
    v = (np.round(np.random.default_rng(116).standard_normal(1 << n) * 1024) / 1024).astype(np.float32)
    want = exact_ref.shapley(v, n)

    def square_error(keep):
        phi = narrow.estimate(keep, v[keep.astype(np.int64)], v[0], v[-1], n, gram="analytic")
        return float(((phi - want) ** 2).mean())

    counter = stream = 0.0
    state = np.random.get_state()
    try:
        for seed in range(1, 21):
            rows, _ = ref.rows(seed, 0, 0, 1000, n)
            counter += square_error(rows[:, 0])
            np.random.seed(seed)
            sizes, orders = narrow.host_draw(n, 1000)
            stream += square_error(narrow.rows_from_orders(orders, sizes, n))
    finally:
        np.random.set_state(state)
    ratio = float(np.sqrt(counter / stream))
    print("RMS error: counter %.5f, stream %.5f, ratio %.4f" % (np.sqrt(counter / 20), np.sqrt(stream / 20), ratio))
    assert 1.0232 - 3 * 0.0858 <= ratio <= 1.0232 + 3 * 0.0858


def test_python_level_refusals_need_no_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    assert wide_kernelshap.DRAWS == ("stream", "counter")
    for bad in ("philox", "", None, "Counter"):
        with pytest.raises(_lib.IqError, match="draw must be one of"):
            wide_kernelshap.game(None, None, None, None, type("A", (), {"num_regions": 128})(), samples=100, draw=bad)
        with pytest.raises(_lib.IqError, match="draw must be one of"):
            wide_kernelshap.shapley(None, None, None, None, type("A", (), {"num_regions": 128})(), samples=100, draw=bad)
    for samples, paired in ((0, False), (1, True), (-4, True)):
        with pytest.raises(_lib.IqError, match="no coalition to draw"):
            wide_kernelshap.draw_counter(128, samples, 1, paired=paired)
    for r in (1, 1025):
        with pytest.raises(_lib.IqError):
            wide_kernelshap.draw_counter(r, 10, 1)


def test_driver_has_the_draw_flag_and_the_sampler_pin_stands():
    from interpret_quality_amd import wide_kernel_stage, wide_stage
    args = wide_kernel_stage.make_args(["--model", "pointnet"])
    assert args.draw == "stream"
    args = wide_kernel_stage.make_args(["--model", "pointnet", "--num_regions", "65", "--draw", "counter", "--seed", "9"])
    assert args.draw == "counter" and args.seed == 9
    with pytest.raises(SystemExit):
        wide_kernel_stage.make_args(["--model", "pointnet", "--draw", "philox"])
    assert wide_stage.SAMPLERS == ("host", "device")
    # under the counter contract a cloud that is not selected draws nothing: no generator, no device
    state = np.random.get_state()
    wide_kernel_stage._skip_draw("unused/", args)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]


def test_draw_counter_is_declared_bound_and_exported_at_abi_116():
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "iq_kshap_draw_counter"
    assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, code) and hasattr(lib, name)
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 116
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "R / 2^32"):
        assert word in header, word
    # argument checks that need no device
    draw = lib.iq_kshap_draw_counter
    assert draw(1, 0, 0, 4, 1, None, 1, None, None, None) == -1 and b"outside 2..1024" in lib.iq_last_error()
    assert draw(1, 0, 0, 4, 1025, None, 1, None, None, None) == -1
    assert draw(1, 0, -1, 4, 128, None, 1, None, None, None) == -1 and b"first" in lib.iq_last_error()
    assert draw(1, 0, (1 << 62) - 3, 4, 128, None, 1, None, None, None) == -1
    assert draw(1, 0, 0, -1, 128, None, 1, None, None, None) == -1
    assert draw(1, 0, 0, (1 << 29) + 1, 128, None, 1, None, None, None) == -1
    assert draw(1, 0, 0, 4, 128, None, 1, None, None, None) == -1 and b"null pointer" in lib.iq_last_error()
    assert draw(1, 0, 0, 0, 128, None, 1, None, None, None) == 0          # S = 0: IQ_OK, nothing read
    assert draw(1, 0, (1 << 62), 0, 128, None, 1, None, None, None) == 0
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_draw_counter(1, 0, 0, 4, 128, device="cpu")
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_draw_counter(1, 0, -1, 4, 128)
