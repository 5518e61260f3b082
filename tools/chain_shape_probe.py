#!/usr/bin/env python3
"""What the bf16 matrix pipe sustains on THIS board per instruction shape: the register-only loops of include/iq_debug.h
(iq_debug_mfma_sustained_shape) on v_mfma_f32_32x32x16_bf16 and v_mfma_f32_16x16x32_bf16, alternately, the 32x32x16 loop first
and last, after warming the board.

    python tools/chain_shape_probe.py [--seconds 1.5] [--pairs 3] [--out profiles/chain_shape_probe.txt]

The chain kernel is power-bound: the ratio of the two rates is the clock the governor gives back for the shape.  The
spread of the repeated 32x32x16 runs is the noise the ratio is read against.
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interpret_quality_amd import _lib  # noqa: E402


def run(lib, shape, seconds, scratch):
    tf, clk = ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(lib.iq_debug_mfma_sustained_shape(shape, float(seconds), ctypes.c_void_p(scratch.data_ptr()), scratch.numel(),
                                                 ctypes.byref(tf), ctypes.byref(clk),
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "iq_debug_mfma_sustained_shape")
    return tf.value, clk.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    scratch = torch.empty(512 * 1024, dtype=torch.float32, device="cuda:0")
    lines = ["# shape  TFLOP/s  shader clock GHz   (%s, %.1f s per run, register-only loop, one wave per SIMD on every CU)"
             % (torch.cuda.get_device_name(0), args.seconds)]
    for shape in (32, 16):      # warm the board: not recorded
        run(lib, shape, args.seconds, scratch)
    res = {32: [], 16: []}
    for shape in [32, 16] * args.pairs + [32]:
        tf, clk = run(lib, shape, args.seconds, scratch)
        res[shape].append(tf)
        lines.append("%-8s %8.1f %8.3f" % ("32x32x16" if shape == 32 else "16x16x32", tf, clk))
        print(lines[-1], flush=True)
    med = {s: sorted(v)[len(v) // 2] for s, v in res.items()}
    lines.append("# median 32x32x16 %.1f (min %.1f, max %.1f), median 16x16x32 %.1f (min %.1f, max %.1f), ratio of medians %.3f"
                 % (med[32], min(res[32]), max(res[32]), med[16], min(res[16]), max(res[16]), med[16] / med[32]))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
