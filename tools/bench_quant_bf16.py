"""QSGD(127, bucket 128) and TernGrad on a bfloat16 gradient against today's workaround and against
the f32 step alone, in one process (no subprocesses), timed with device events.  Per codec:

  step      the fused world-1 step             bf16: ops.*_step_w1(g)
                                               cast: ops.*_step_w1(g.float()).to(bfloat16)
                                               f32 : ops.*_step_w1(g32)
  compress  codes + norms / scalars alone      bf16: ops.*_compress(g)
                                               cast: ops.*_compress(g.float())
                                               f32 : ops.*_compress(g32)
  decode    W = 8 rank-major int8 payloads,    bf16: ops.*_decompress(..., out_dtype=bfloat16)
            decoded, summed and averaged       cast: ops.*_decompress(...).to(bfloat16)

Bytes per element are counted from the launches' arguments, not measured.  Two
inputs: the 161 tensors of ResNet-50 as one segmented bucket, and one tensor of 2^26 elements; each
has three rotated gradients, as bench.py rotates its buffers, and every row is warmed up before it is
timed.  The variants of a row group alternate in rounds of --steps calls; each row reports the
median, fastest and slowest round in microseconds per call, the bytes moved and the share of the
8 TB/s peak that is.

    python tools/bench_quant_bf16.py [--inputs resnet50,67108864] [--rounds R] [--steps S] [--out FILE]
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
Q = 127
PEAK = 8e12
BF16 = torch.bfloat16
# bytes per element: (bf16, cast, f32)
BYTES = {("qsgd", "step"): (4, 20, 8), ("tern", "step"): (6, 24, 12),
         ("qsgd", "compress"): (3, 11, 5), ("tern", "compress"): (5, 15, 9),
         ("qsgd", "decode"): (W + 2, W + 10, None), ("tern", "decode"): (W + 2, W + 10, None)}


def resnet50_sizes():
    import bench
    sizes = []
    for s in bench.resnet50_shapes():
        k = 1
        for d in s:
            k *= d
        sizes.append(k)
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default=f"resnet50,{1 << 26}")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(dev)}: {args.rounds} rounds of {args.steps} calls per row, us per call "
             f"(median, min, max of the rounds); bytes counted, share of {PEAK / 1e12:.0f} TB/s; decode rows: W = {W}",
             f"{'input':>10} {'row':<20}{'B/elem':>7}{'median us':>11}{'min':>10}{'max':>10}{'MB moved':>10}{'of peak':>9}"]
    ratios = []
    for inp in args.inputs.split(","):
        sizes = resnet50_sizes() if inp == "resnet50" else [int(inp)]
        n = sum(sizes)
        gen = torch.Generator(device=dev)
        g16, g32 = [], []
        for j in range(3):
            gen.manual_seed(j + 1)
            g16.append((torch.randn(n, device=dev, generator=gen) * 0.01).to(BF16))
            g32.append(g16[-1].float())
        # W rank-major payloads (the three gradients in turn, different seeds)
        qp = [ops.qsgd_compress(g16[w % 3], Q, 128, sizes=sizes, seed=100 + w) for w in range(W)]
        qcodes, qnorms = torch.cat([p[0] for p in qp]), torch.cat([p[1] for p in qp])
        tp = [ops.terngrad_compress(g16[w % 3], sizes=sizes, seed=100 + w) for w in range(W)]
        tcodes, tscal = torch.cat([p[0] for p in tp]), torch.cat([p[1] for p in tp])
        del qp, tp
        qdec = dict(sizes=sizes, world=W, aggregate=True, divisor=float(W))
        rows = {
            ("qsgd", "step"): (lambda i: ops.qsgd_step_w1(g16[i % 3], Q, sizes=sizes, seed=i),
                               lambda i: ops.qsgd_step_w1(g16[i % 3].float(), Q, sizes=sizes, seed=i).to(BF16),
                               lambda i: ops.qsgd_step_w1(g32[i % 3], Q, sizes=sizes, seed=i)),
            ("qsgd", "compress"): (lambda i: ops.qsgd_compress(g16[i % 3], Q, 128, sizes=sizes, seed=i),
                                   lambda i: ops.qsgd_compress(g16[i % 3].float(), Q, 128, sizes=sizes, seed=i),
                                   lambda i: ops.qsgd_compress(g32[i % 3], Q, 128, sizes=sizes, seed=i)),
            ("qsgd", "decode"): (lambda i: ops.qsgd_decompress(qcodes, qnorms, Q, 128, n, out_dtype=BF16, **qdec),
                                 lambda i: ops.qsgd_decompress(qcodes, qnorms, Q, 128, n, **qdec).to(BF16)),
            ("tern", "step"): (lambda i: ops.terngrad_step_w1(g16[i % 3], sizes=sizes, seed=i),
                               lambda i: ops.terngrad_step_w1(g16[i % 3].float(), sizes=sizes, seed=i).to(BF16),
                               lambda i: ops.terngrad_step_w1(g32[i % 3], sizes=sizes, seed=i)),
            ("tern", "compress"): (lambda i: ops.terngrad_compress(g16[i % 3], sizes=sizes, seed=i),
                                   lambda i: ops.terngrad_compress(g16[i % 3].float(), sizes=sizes, seed=i),
                                   lambda i: ops.terngrad_compress(g32[i % 3], sizes=sizes, seed=i)),
            ("tern", "decode"): (lambda i: ops.terngrad_decompress(tcodes, tscal, n, out_dtype=BF16, **qdec),
                                 lambda i: ops.terngrad_decompress(tcodes, tscal, n, **qdec).to(BF16)),
        }
        for key, fns in rows.items():
            for i in range(args.warmup):
                for f in fns:
                    f(i)
            us = [[] for _ in fns]
            for _ in range(args.rounds):
                for v, f in enumerate(fns):      # the variants of one row group alternate
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(args.steps):
                        f(i)
                    e1.record()
                    e1.synchronize()
                    us[v].append(e0.elapsed_time(e1) / args.steps * 1e3)
            med = [statistics.median(u) for u in us]
            for v, name in enumerate(("bf16", "cast", "f32")[:len(fns)]):
                moved = BYTES[key][v] * n
                lines.append(f"{inp:>10} {key[0] + ' ' + key[1] + ' ' + name:<20}{BYTES[key][v]:>7}{med[v]:>11.1f}"
                             f"{min(us[v]):>10.1f}{max(us[v]):>10.1f}{moved / 1e6:>10.1f}"
                             f"{moved / (med[v] * 1e-6) / PEAK:>9.1%}")
            ratios.append(f"{inp}: {key[0]} {key[1]}: cast / bf16 = {med[1] / med[0]:.2f}x" +
                          (f", f32 / bf16 = {med[2] / med[0]:.2f}x" if len(fns) == 3 else ""))
        del g16, g32, qcodes, qnorms, tcodes, tscal, rows
        torch.cuda.empty_cache()
    text = "\n".join(lines + ratios) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
