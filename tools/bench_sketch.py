"""The quantile-bucket quantiser (grace_amd/csrc/sketch.hip) at 2^26 elements, f32 and
bf16, 16 and 256 buckets, in one process, timed with device events:

  edges      ops.sketch_edges                         the multi-select alone
  compress   ops.sketch_compress                      codes + means
  step       ops.sketch_step_w1                       the world-1 step, dense result in g's dtype
  decode     ops.sketch_decode_aggregate, W = 8       rank-major payloads, averaged, result in g's dtype

Beside each row: (a) the row's bytes over 8 TB/s, counted from the launches' arguments, not measured (a
select pass reads x once: four passes on f32, two on bf16; the encode reads x and writes the codes; the
step then reads the codes and writes the result); (b) the eager-PyTorch composition a user has without
the codec (torch.sort, an index, bucketize, index_add_, a division and a gather) on the same buffers;
(c) for the decode at 256 buckets, ops.u8bit_decode_aggregate, which moves the same bytes.  The variants
of a row alternate in rounds of --steps calls (a tenth of them for the eager composition); each reports
the median, fastest and slowest round in microseconds per call.  A variant whose warm-up call takes over
a quarter of a second is not repeated: the wall time of that call is its one figure.

    python tools/bench_sketch.py [--n N] [--rounds R] [--steps S] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grace_amd import ops  # noqa: E402

W = 8
PEAK = 8e12


def eager_edges(g, q):
    xs = torch.sort(g.float().view(-1)).values
    return xs[(torch.arange(q + 1, device=g.device) * (xs.numel() - 1)) // q]


def eager_compress(g, q):
    x = g.float().view(-1)
    codes = torch.bucketize(x, eager_edges(g, q)[1:q].contiguous(), right=True)
    sums = torch.zeros(q, dtype=torch.float64, device=g.device).index_add_(0, codes, x.double())
    means = (sums / torch.bincount(codes, minlength=q).clamp_(min=1)).float()
    return codes.to(torch.uint8), means


def eager_step(g, q):
    codes, means = eager_compress(g, q)
    return (0 + means[codes.long()]).to(g.dtype)


def eager_decode(codes, means, n, q, dtype):
    """W rank-major payloads of one byte a code, summed in rank order and averaged"""
    acc = torch.zeros(n, device=codes.device)
    for w in range(W):
        acc = acc + means[w * q:(w + 1) * q][codes[w * n:(w + 1) * n].long()]
    return (acc / W).to(dtype)


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
    head = [f"{torch.cuda.get_device_name(dev)}: n = {n}, {args.rounds} rounds of {args.steps} calls per row, us per "
             f"call (median, min, max of the rounds); bytes counted; (a) = bytes / {PEAK / 1e12:.0f} TB/s; decode: W = {W}",
             f"{'row':<38}{'B/elem':>7}{'(a) us':>9}{'median us':>13}{'min':>13}{'max':>13}{'of peak':>9}"]
    for h in head:
        emit(h)
    ratios = []
    gen = torch.Generator(device=dev).manual_seed(1)
    g32 = [torch.randn(n, device=dev, generator=gen) * 0.01 for _ in range(3)]
    u8_values = ops.u8bit_tables("floor")[1]
    for dtype, name, sz in ((torch.float32, "f32", 4), (torch.bfloat16, "bf16", 2)):
        g = g32 if sz == 4 else [t.to(dtype) for t in g32]
        sel = sz * (4 if sz == 4 else 2)             # the select's reads of x
        for q in (16, 256):
            cb = 1.0 if q > 16 else 0.5
            pay = [ops.sketch_compress(g[w % 3], q) for w in range(W)]
            codes, means = torch.cat([p[0] for p in pay]), torch.cat([p[1] for p in pay])
            bytecodes = codes if q > 16 else torch.stack([codes & 15, codes >> 4], 1).view(-1)   # for (b)
            del pay
            rows = {
                "edges": (sel, [lambda i: ops.sketch_edges(g[i % 3], q), lambda i: eager_edges(g[i % 3], q)]),
                "compress": (sel + sz + cb, [lambda i: ops.sketch_compress(g[i % 3], q),
                                             lambda i: eager_compress(g[i % 3], q)]),
                "step": (sel + 2 * sz + 2 * cb, [lambda i: ops.sketch_step_w1(g[i % 3], q),
                                                 lambda i: eager_step(g[i % 3], q)]),
                "decode": (W * cb + sz, [
                    lambda i: ops.sketch_decode_aggregate(codes, means, W, n, q, divisor=float(W), out_dtype=dtype),
                    lambda i: eager_decode(bytecodes, means, n, q, dtype)]),
            }
            if q > 16:
                i8, scales = codes.view(torch.int8), torch.ones(W, device=dev)
                rows["decode"][1].append(lambda i: ops.u8bit_decode_aggregate(i8, scales, W, n, 0, u8_values,
                                                                              divisor=float(W), out_dtype=dtype))
            med_of = {}
            for row, (bpe, fns) in rows.items():
                steps = [args.steps, max(1, args.steps // 10), args.steps]
                us = [[] for _ in fns]
                for v, f in enumerate(fns):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(args.warmup):
                        f(i)
                    torch.cuda.synchronize()
                    once = (time.perf_counter() - t0) / args.warmup
                    if once > 0.25:                  # too slow to repeat: the warm-up's wall time stands for it
                        us[v].append(once * 1e6)
                for _ in range(args.rounds):
                    for v, f in enumerate(fns):      # the variants of one row alternate
                        if len(us[v]) == 1 and us[v][0] > 0.25e6:
                            continue
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(steps[v]):
                            f(i)
                        e1.record()
                        e1.synchronize()
                        us[v].append(e0.elapsed_time(e1) / steps[v] * 1e3)
                med = med_of[row] = [statistics.median(u) for u in us]
                tag = f"{name} q {q} {row}"
                for v, what in enumerate(("sketch", "(b) eager", "(c) u8bit decode")[:len(fns)]):
                    b = bpe if v != 1 else None
                    floor = f"{b * n / PEAK * 1e6:>9.1f}" if b else f"{'':>9}"
                    peak = f"{b * n / (med[v] * 1e-6) / PEAK:>9.1%}" if b else ""
                    emit(f"{tag + ' ' + what:<38}{(f'{b:.1f}' if b else ''):>7}{floor}{med[v]:>13.1f}"
                         f"{min(us[v]):>13.1f}{max(us[v]):>13.1f}{peak}")
                ratios.append(f"{tag}: sketch / (a) = {med[0] / (bpe * n / PEAK * 1e6):.2f}x, (b) / sketch = "
                              f"{med[1] / med[0]:.1f}x" + (f", sketch / (c) = {med[0] / med[2]:.2f}x" if len(fns) > 2 else ""))
            ratios.append(f"{name} q {q}: the select is {med_of['edges'][0] / med_of['compress'][0]:.0%} of compress")
            del codes, means, bytecodes
            torch.cuda.empty_cache()
    print("\n".join(ratios), flush=True)
    text = "\n".join(lines + ratios) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
