"""The microscaling codec (grace_amd/csrc/mx.hip) at 2^26 elements, f32 and bf16, the
five formats and both roundings, in one process, timed with device events, on a normal gradient of scale 1e-3:

  compress   ops.mx_compress                     the fixed-size payload
  step       ops.mx_step_w1                      the world-1 step, dense result in g's dtype
  decode     ops.mx_decode_aggregate, W = 8      eight payloads, averaged, result in g's dtype (once a format:
                                                 the decode does not know the rounding)

Beside each row: the row's bytes counted from the launch's arguments, not measured (compress reads sz * n and
writes n * bits / 8 + n / 32; the step writes sz * n instead; the decode reads W payloads and writes sz * n),
those bytes over 8 TB/s, and the rate they imply.  In the same run and on the same tensors, per dtype: the
8-bit elementwise codec (natural_compress, natural_decompress at W = 8) and the block-wise 8-bit codebook
encode (u8bit_compress, blocks of 256).  The gradient rotates over three buffers; the rows of a dtype
alternate in rounds of --steps calls; each reports the median, fastest and slowest round in microseconds
per call, and the MX rows their time over the natural codec's.

    python tools/bench_mx.py [--n N] [--rounds R] [--steps S] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grace_amd import ops  # noqa: E402

W = 8
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    emit(f"{torch.cuda.get_device_name(dev)}: n = {n}, {args.rounds} rounds of {args.steps} calls per row, us per call "
         f"(median, min, max of the rounds); bytes counted; floor = bytes / {PEAK / 1e12:.0f} TB/s; decode: W = {W}")
    emit(f"{'row':<44}{'B/elem':>8}{'floor us':>10}{'median us':>11}{'min':>9}{'max':>9}{'TB/s':>7}{'of peak':>9}"
         f"{'/ natural':>10}")
    gen = torch.Generator(device=dev).manual_seed(1)
    base = [torch.randn(n, device=dev, generator=gen) * 1e-3 for _ in range(3)]
    edges = ops.u8bit_tables("floor")[0]
    for dtype, name, sz in ((torch.float32, "f32", 4), (torch.bfloat16, "bf16", 2)):
        g = [t.to(dtype) for t in base]
        nat = torch.cat([ops.natural_compress(g[w % 3], seed=w) for w in range(W)])
        rows = [   # (tag, bytes per element, call, the reference row its time is divided by)
            ("natural compress", sz + 1, lambda i: ops.natural_compress(g[i % 3], seed=i), None),
            ("natural decode", W + sz, lambda i: ops.natural_decompress(nat, n, 0, world=W, aggregate=True,
                                                                        divisor=float(W), out_dtype=dtype), None),
            ("u8bit compress block 256", sz + 1 + 4 / 256, lambda i: ops.u8bit_compress(g[i % 3], 256, edges), None)]
        wires = {}
        for fmt, bits in zip(ops.MX_FORMATS, ops.MX_BITS):
            wire = bits / 8 + 1 / 32
            wires[fmt] = torch.cat([ops.mx_compress(g[w % 3], fmt) for w in range(W)])
            for rounding in ops.MX_ROUNDINGS:
                rows.append((f"{fmt} {rounding} compress", sz + wire,
                             lambda i, f=fmt, r=rounding: ops.mx_compress(g[i % 3], f, r, seed=i), 0))
                rows.append((f"{fmt} {rounding} step", 2 * sz,
                             lambda i, f=fmt, r=rounding: ops.mx_step_w1(g[i % 3], f, r, seed=i), 0))
            rows.append((f"{fmt} decode", W * wire + sz,
                         lambda i, f=fmt: ops.mx_decode_aggregate(wires[f], W, n, f, divisor=float(W), out_dtype=dtype), 1))
        us = [[] for _ in rows]
        for _, _, f, _ in rows:
            for i in range(args.warmup):
                f(i)
        for _ in range(args.rounds):
            for v, (_, _, f, _) in enumerate(rows):          # the rows alternate
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.steps):
                    f(i)
                e1.record()
                e1.synchronize()
                us[v].append(e0.elapsed_time(e1) / args.steps * 1e3)
        med = [statistics.median(u) for u in us]
        for v, (tag, bpe, _, ref) in enumerate(rows):
            rate = bpe * n / (med[v] * 1e-6)
            emit(f"{name + ' ' + tag:<44}{bpe:>8.3f}{bpe * n / PEAK * 1e6:>10.1f}{med[v]:>11.1f}{min(us[v]):>9.1f}"
                 f"{max(us[v]):>9.1f}{rate / 1e12:>7.2f}{rate / PEAK:>9.1%}"
                 + (f"{med[v] / med[ref]:>9.2f}x" if ref is not None else ""))
        del g, nat, wires, rows
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
