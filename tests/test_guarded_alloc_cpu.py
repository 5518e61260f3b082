"""CPU: tests/guarded_alloc.py catches what it claims, and the table of tests/test_workspace_contents_gpu.py is complete.

The helper's classes take a device.  Here they run on CPU tensors against toy "library calls" - one that reads an accumulator
it never cleared, one that writes a byte behind the size it asked for, one that writes a byte in front, and a correct one - so a
reader without a GPU can see that the GPU test bites: it uses the same classes, only the device differs.  Raw-pointer writes are
played by ``torch.as_strided`` on the body, which reaches the bytes around it as a pointer would.

Completeness: every package module whose source calls ``torch.empty(`` is patched by ``guarded_empty`` or exempt with a reason, and
every public ``hip_ops`` function that allocates (itself or through a private helper) has a row in the GPU test's ``OPS`` table."""
import inspect
import pathlib
import re

import pytest
import torch

import guarded_alloc as G
from interpret_quality_amd import hip_ops, workspace

N = 64          # bytes the toy calls ask for


def toy_correct(ws, x):
    acc = ws[:8].view(torch.float64)
    acc.zero_()
    acc += x.double().sum()
    return acc.clone()


def toy_missing_clear(ws, x):
    acc = ws[:8].view(torch.float64)        # never cleared: whatever the memory held is part of the sum
    acc += x.double().sum()
    return acc.clone()


def toy_overrun(ws, x):
    torch.as_strided(ws, (ws.numel() + 1,), (1,))[-1] = 7           # one byte behind the size asked
    return toy_correct(ws, x)


def toy_underrun(ws, x):
    torch.as_strided(ws, (1,), (1,), ws.storage_offset() - 1)[0] = 7          # one byte in front
    return toy_correct(ws, x)


X, X_DONOR = torch.arange(5.0), torch.arange(5.0) + 0.5


def run(call, fill, x=X):
    g = G.Guarded(N, fill, "cpu")
    out = call(g.body, x)
    g.check()
    return out, g


def stale_of(call):
    """A STALE fill from what ``call`` on other inputs left in its buffer of the same size."""
    return G.STALE(run(call, G.ZERO, X_DONOR)[1])


def test_guard_layout():
    g = G.Guarded(N, G.ONES, "cpu")
    assert G.GUARD == 4 << 20 and G.GUARD % 256 == 0
    assert g.buf.numel() == 2 * G.GUARD + N and g.body.numel() == N and g.body.storage_offset() == G.GUARD
    assert bool((g.body == 0xFF).all()) and all(bool((t == 0xA5).all()) for _, t in g.guards())
    assert bool((G.Guarded(N, G.ZERO, "cpu").body == 0).all())
    assert G.Guarded(0, G.ONES, "cpu").body.numel() == 0
    donor = G.Guarded(N, G.ZERO, "cpu")
    donor.body.copy_(torch.arange(N, dtype=torch.uint8))
    assert torch.equal(G.Guarded(N, G.STALE(donor), "cpu").body, donor.body)


def test_a_correct_call_passes_all_three_fills():
    want = toy_correct(torch.zeros(N, dtype=torch.uint8), X)
    for fill in (G.ZERO, G.ONES, stale_of(toy_correct)):
        assert torch.equal(run(toy_correct, fill)[0], want)


def test_a_missing_clear_shows_between_zero_and_stale():
    zero = run(toy_missing_clear, G.ZERO)[0]
    stale = run(toy_missing_clear, stale_of(toy_missing_clear))[0]
    assert torch.equal(zero, toy_correct(torch.zeros(N, dtype=torch.uint8), X))     # ZERO alone cannot see it
    assert not torch.equal(stale, zero)
    ones = run(toy_missing_clear, G.ONES)[0]
    assert not torch.equal(ones.view(torch.int64), zero.view(torch.int64))          # a NaN here; an int max merge would hide from ONES


def test_one_byte_past_the_end_names_the_tail_guard_and_offset_0():
    with pytest.raises(G.GuardError, match=r"tail guard .* changed at offset 0 of"):
        run(toy_overrun, G.ZERO)


def test_one_byte_in_front_names_the_front_guard():
    with pytest.raises(G.GuardError, match=r"front guard .* changed at offset %d of" % (G.GUARD - 1)):
        run(toy_underrun, G.ZERO)


class ToyEngine:
    device = torch.device("cpu")

    def __init__(self):
        self._ws, self.replaced = None, 0

    def workspace_replaced(self):
        self.replaced += 1

    def call(self, nbytes, body=toy_correct, x=X):
        return body(workspace.ensure(self, nbytes), x)        # reached as a module attribute, as the engines reach it


def test_guarded_workspaces_hands_out_fresh_exact_bodies_and_checks_them():
    eng, real = ToyEngine(), workspace.ensure
    with G.guarded_workspaces(G.ONES) as rec:
        eng.call(N)
        first = eng._ws
        eng.call(N)
        assert eng._ws is not first and eng._ws.numel() == N and eng.replaced == 2
    assert workspace.ensure is real and eng._ws is None and eng.replaced == 3
    assert rec.sizes() == [N, N] and rec.workspaces == list(rec)
    with pytest.raises(G.GuardError, match="tail guard of workspace 1 of ToyEngine"):
        with G.guarded_workspaces(G.ZERO):
            eng.call(N)
            eng.call(N, toy_overrun)
    assert workspace.ensure is real


def test_stale_replays_the_donor_run_allocation_by_allocation():
    eng = ToyEngine()
    with G.guarded_workspaces(G.ZERO) as donor:
        eng.call(N, x=X_DONOR)
        eng.call(2 * N, x=X_DONOR)
    with G.guarded_workspaces(G.STALE(donor)):
        a = eng.call(N, toy_missing_clear)
        eng.call(2 * N)
    assert float(a) == float(X.sum() + X_DONOR.sum())          # the donor's sum was still there
    with pytest.raises(AssertionError, match="the donor's buffer has"):
        with G.guarded_workspaces(G.STALE(donor)):
            eng.call(N + 1)
    with pytest.raises(AssertionError, match="made 1 allocations, the donor 2"):
        with G.guarded_workspaces(G.STALE(donor)):
            eng.call(N)


def test_guarded_empty_proxies_the_patched_modules_only():
    real = torch.empty
    with G.guarded(G.ONES, device_type="cpu") as rec:
        assert torch.empty is real and hip_ops.torch is not torch and hip_ops.torch.float32 is torch.float32
        t = hip_ops.torch.empty((3, 5), dtype=torch.int32, device="cpu")
        u = hip_ops.torch.empty(7, dtype=torch.float64, device=torch.device("cpu"))
        plain = hip_ops.torch.empty((2,), dtype=torch.int32)           # no device named: a host-side array, passed through
        assert t.shape == (3, 5) and t.dtype == torch.int32 and bool((t == -1).all()) and u.shape == (7,) and bool(torch.isnan(u).all())
        assert rec.sizes() == [60, 56] and plain.shape == (2,)
        t.zero_()
    assert hip_ops.torch is torch
    with pytest.raises(G.GuardError, match=r"tail guard of torch.empty 0: \(4,\)"):
        with G.guarded_empty(G.ZERO, device_type="cpu"):
            t = hip_ops.torch.empty((4,), dtype=torch.float32, device="cpu")
            torch.as_strided(t, (5,), (1,))[4] = 1.0
    assert hip_ops.torch is torch


# ---- completeness ------------------------------------------------------------------------------------------------------------

PKG = pathlib.Path(hip_ops.__file__).parent
# modules that call torch.empty( and are NOT patched by guarded_empty, each with its reason
EXEMPT = {
    "workspace": "its one torch.empty is workspace.ensure itself, which guarded_workspaces replaces as a whole",
    "dist": "the receive buffer of torch.distributed.all_gather_into_tensor: no library call reads or writes it",
}
# public hip_ops functions that allocate and have no row in OPS, each with its reason
EXEMPT_OPS = {}


def test_every_module_that_calls_torch_empty_is_patched_or_exempt():
    hits = {p.stem for p in PKG.glob("*.py") if "torch.empty(" in p.read_text()}
    assert "hip_ops" in hits and "engine" in hits
    assert hits == set(G.PATCHED_MODULES) | set(EXEMPT), sorted(hits ^ (set(G.PATCHED_MODULES) | set(EXEMPT)))
    assert not set(G.PATCHED_MODULES) & set(EXEMPT) and all(EXEMPT.values())


def allocating_ops():
    """Public hip_ops functions whose source calls torch.empty( or a private helper that does (transitively)."""
    funcs = {n: inspect.getsource(f) for n, f in vars(hip_ops).items() if inspect.isfunction(f) and f.__module__ == hip_ops.__name__}
    alloc = {n for n, src in funcs.items() if "torch.empty(" in src}
    while True:
        private = [n for n in alloc if n.startswith("_")]
        more = {n for n, src in funcs.items() if n not in alloc and any(re.search(r"\b%s\(" % re.escape(p), src) for p in private)}
        if not more:
            return {n for n in alloc if not n.startswith("_")}
        alloc |= more


def test_every_allocating_wrapper_has_a_row_in_the_gpu_table():
    import test_workspace_contents_gpu as W        # importing it touches no GPU
    need = allocating_ops()
    assert {"knn", "shapley_accum", "shapley_accum_wide", "exact_shapley", "kshap_keep_masks_wide", "linear"} <= need    # the scan sees helpers
    covered = {wrapper for _, wrapper, _ in W.OPS}
    assert all(hasattr(hip_ops, w) for w in covered)
    missing = need - covered - set(EXEMPT_OPS)
    assert not missing, sorted(missing)
    assert not set(EXEMPT_OPS) & covered and all(EXEMPT_OPS.values())
