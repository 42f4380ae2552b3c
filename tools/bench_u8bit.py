"""The 8-bit codebook quantiser (grace_amd/csrc/u8bit.hip) at 2^26 elements, f32
and bf16, block 0 (one scale) and 4096, in one process, timed with device events:

  compress   ops.u8bit_compress                      codes + scales
  step       ops.u8bit_step_w1                       the fused world-1 step, dense result in g's dtype
  decode     ops.u8bit_decode_aggregate, W = 8       rank-major payloads, averaged, result in g's dtype

Beside each row: (a) the row's algorithmic bytes over 8 TB/s; (b) the same-traffic kernel already in the
tree on the same buffers -- ops.natural_compress (4 -> 1 or 2 -> 1 bytes an element), ops.cast_step_w1
(4 -> 4, 2 -> 2) and ops.natural_decompress (W + 4, W + 2); (c) an eager-PyTorch composition of the
same arithmetic (abs().amax, division, torch.bucketize, gather), which is what a user has without
the codec.  Bytes are counted from the launches' arguments, not measured: a tensor-wide encode reads
x twice.  The variants of a row alternate in rounds of --steps calls; each reports the median,
fastest and slowest round in microseconds per call.

    python tools/bench_u8bit.py [--n N] [--rounds R] [--steps S] [--out FILE]
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


def eager_encode(g, block, edges):
    x = g.float()
    X = x.view(-1, block) if block else x.view(1, -1)
    a = X.abs().amax(dim=1)
    i = (torch.bucketize(X.abs() / a[:, None], edges, right=True) - 1).clamp_(min=0)
    return torch.where(X < 0, -i, i).to(torch.int8).view(-1), a


def eager_decode(codes, scales, block, values, n):
    """W rank-major payloads, summed in rank order and averaged"""
    acc = torch.zeros(n, device=codes.device)
    for w in range(W):
        c = codes[w * n:(w + 1) * n].view(-1, block) if block else codes[w * n:(w + 1) * n].view(1, -1)
        nb = c.shape[0]
        mag = values[c.abs().long()] * scales[w * nb:(w + 1) * nb, None]
        acc = acc + torch.where(c < 0, -mag, mag).view(-1)
    return acc / W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    edges, values = ops.u8bit_tables("floor")
    lines = [f"{torch.cuda.get_device_name(dev)}: n = {n}, {args.rounds} rounds of {args.steps} calls per row, us per "
             f"call (median, min, max of the rounds); bytes counted; (a) = bytes / {PEAK / 1e12:.0f} TB/s; decode: W = {W}",
             f"{'row':<34}{'B/elem':>7}{'(a) us':>9}{'median us':>11}{'min':>9}{'max':>9}{'of peak':>9}"]
    ratios = []
    gen = torch.Generator(device=dev).manual_seed(1)
    g32 = [torch.randn(n, device=dev, generator=gen) * 0.01 for _ in range(3)]
    for dtype, name, sz in ((torch.float32, "f32", 4), (torch.bfloat16, "bf16", 2)):
        g = g32 if sz == 4 else [t.to(dtype) for t in g32]
        nat = torch.cat([ops.natural_compress(g[w % 3], seed=w) for w in range(W)])
        for block in (0, 4096):
            pay = [ops.u8bit_compress(g[w % 3], block, edges) for w in range(W)]
            codes, scales = torch.cat([p[0] for p in pay]), torch.cat([p[1] for p in pay])
            del pay
            sb = 4.0 / block if block else 0.0
            rows = {
                "compress": ((2 * sz if block == 0 else sz) + 1 + sb, sz + 1, [
                    lambda i: ops.u8bit_compress(g[i % 3], block, edges),
                    lambda i: ops.natural_compress(g[i % 3], seed=i),
                    lambda i: eager_encode(g[i % 3], block, edges)]),
                "step": ((3 * sz if block == 0 else 2 * sz) + sb, 2 * sz, [
                    lambda i: ops.u8bit_step_w1(g[i % 3], block, edges, values),
                    lambda i: ops.cast_step_w1(g[i % 3], 0, i),
                    lambda i: eager_step(g[i % 3], block, edges, values)]),
                "decode": (W + sz + W * sb, W + sz, [
                    lambda i: ops.u8bit_decode_aggregate(codes, scales, W, n, block, values, divisor=float(W),
                                                         out_dtype=dtype),
                    lambda i: ops.natural_decompress(nat, n, 0, world=W, aggregate=True, divisor=float(W),
                                                     out_dtype=dtype),
                    lambda i: eager_decode(codes, scales, block, values, n).to(dtype)]),
            }
            for row, (bpe, bpe_ref, fns) in rows.items():
                steps = [args.steps, args.steps, max(1, args.steps // 10)]     # the eager composition is slow
                for i in range(args.warmup):
                    for f in fns:
                        f(i)
                us = [[] for _ in fns]
                for _ in range(args.rounds):
                    for v, f in enumerate(fns):      # the variants of one row alternate
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(steps[v]):
                            f(i)
                        e1.record()
                        e1.synchronize()
                        us[v].append(e0.elapsed_time(e1) / steps[v] * 1e3)
                med = [statistics.median(u) for u in us]
                tag = f"{name} block {block} {row}"
                for v, (what, b) in enumerate((("u8bit", bpe), ("(b) same traffic", bpe_ref), ("(c) eager", None))):
                    floor = f"{b * n / PEAK * 1e6:>9.1f}" if b else f"{'':>9}"
                    peak = f"{b * n / (med[v] * 1e-6) / PEAK:>9.1%}" if b else ""
                    lines.append(f"{tag + ' ' + what:<34}{(f'{b:.3f}' if b else ''):>7}{floor}{med[v]:>11.1f}"
                                 f"{min(us[v]):>9.1f}{max(us[v]):>9.1f}{peak}")
                ratios.append(f"{tag}: u8bit / (a) = {med[0] / (bpe * n / PEAK * 1e6):.2f}x, u8bit / (b) = "
                              f"{med[0] / med[1]:.2f}x, (c) / u8bit = {med[2] / med[0]:.1f}x")
            del codes, scales
        del nat
        torch.cuda.empty_cache()
    text = "\n".join(lines + ratios) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def eager_step(g, block, edges, values):
    codes, a = eager_encode(g, block, edges)
    c = codes.view(-1, block) if block else codes.view(1, -1)
    mag = values[c.abs().long()] * a[:, None]
    return (0 + torch.where(c < 0, -mag, mag)).view(-1).to(g.dtype)


if __name__ == "__main__":
    main()
