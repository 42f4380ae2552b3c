"""Threshold and random-k on a bfloat16 gradient against today's workaround (cast up, the f32 class's
step, cast down), in one process, timed with device events.

  threshold      Allgather(ThresholdCompressor(thr), ResidualMemory(), 1).step, the threshold at the
                 gradient's 1 % quantile, steady state (the residual carried), 2^26 elements
                                bf16: grace_amd.sparse_bf16's class on g
                                cast: grace_amd.dist's class on g.float(), then .to(bfloat16)
  threshold -m   the same with NoneMemory
  randomk        Allgather(RandomKCompressor(0.01), ResidualMemory(), 1).step, the same two variants
  decode         the W = 8 padded buffers of a threshold counts exchange (1 % to 6 % per rank), summed
                 and averaged, at 2^26 and at 50,000 (launch bound: reported only)
                                bf16: ops.sparse_aggregate_padded(...)
                                cast: ops.f32_to_bf16(ops.sparse_aggregate(...))

Bytes are counted from the launches' arguments, not measured; the index grouping
of random-k and the threshold's per-chunk partials (under 1 % of a step's bytes) are left out.  Three
rotated gradients, as bench.py rotates its buffers; every row is warmed up before it is timed; the
two variants of a row alternate in rounds of --steps calls; each row reports the median, fastest and
slowest round in microseconds per call, the bytes moved and the share of the 8 TB/s peak.

    python tools/bench_sparse_bf16.py [--n 67108864] [--rounds R] [--steps S] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grace_amd import ops, sparse_bf16  # noqa: E402
from grace_amd.dist.communicator.allgather import Allgather  # noqa: E402
from grace_amd.dist.compressor.randomk import RandomKCompressor  # noqa: E402
from grace_amd.dist.compressor.threshold import ThresholdCompressor  # noqa: E402
from grace_amd.dist.memory.none import NoneMemory  # noqa: E402
from grace_amd.dist.memory.residual import ResidualMemory  # noqa: E402

W = 8
RATIO = 0.01
SIGMA = 0.01
THR = 2.5758 * SIGMA     # |x| above it: 1 % of N(0, sigma^2)
PEAK = 8e12
BF16 = torch.bfloat16
NAMES = ("bf16", "cast")


class Step:
    """One variant of a steady-state step: its own communicator, so its own carried residual."""

    def __init__(self, grads, comm, cast):
        self.g, self.comm, self.cast = grads, comm, cast

    def __call__(self, i):
        g = self.g[i % 3]
        if self.cast:
            return self.comm.step(g.float(), "w").to(BF16)
        return self.comm.step(g, "w")


def padded(g32, n, dev):
    """The W padded buffers of a counts exchange (the three gradients in turn, scaled apart): (buffer,
    cap, device counts, host counts)."""
    sel = [ops.threshold_compress(g32[w % 3] * (1.0 + 0.05 * w), THR) for w in range(W)]
    counts = [v.numel() for v, _ in sel]
    cap = max(max(counts), 1)
    buf = torch.zeros(W, 2 * cap, dtype=torch.float32, device=dev)
    for w, (v, i) in enumerate(sel):
        buf[w, :counts[w]] = v
        buf[w, cap:cap + counts[w]] = i.view(torch.float32)
    return buf.view(-1), cap, torch.tensor(counts, dtype=torch.int32, device=dev), counts


def time_rows(fns, args):
    for i in range(args.warmup):
        for f in fns:
            f(i)
    us = [[] for _ in fns]
    for _ in range(args.rounds):
        for v, f in enumerate(fns):      # the variants of one row alternate
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                f(i)
            e1.record()
            e1.synchronize()
            us[v].append(e0.elapsed_time(e1) / args.steps * 1e3)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--decode-sizes", default=f"{1 << 26},50000")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(dev)}: {args.rounds} rounds of {args.steps} calls per row, us per call "
             f"(median, min, max of the rounds); bytes counted, share of {PEAK / 1e12:.0f} TB/s; decode rows: W = {W}",
             f"{'n':>10} {'row':<30}{'median us':>11}{'min':>10}{'max':>10}{'MB moved':>10}{'of peak':>9}"]
    verdicts = []

    def report(n, row, us, moved):
        med = [statistics.median(u) for u in us]
        for v, u in enumerate(us):
            lines.append(f"{n:>10} {row + ' ' + NAMES[v]:<30}{med[v]:>11.1f}{min(u):>10.1f}{max(u):>10.1f}"
                         f"{moved[v] / 1e6:>10.1f}{moved[v] / (med[v] * 1e-6) / PEAK:>9.1%}")
        verdicts.append(f"{n}: {row}: bf16 median {med[0]:.1f} us against the cast row's fastest round "
                        f"{min(us[1]):.1f} us ({'below' if med[0] < min(us[1]) else 'NOT below'}); cast / bf16 = "
                        f"{med[1] / med[0]:.2f}x (bytes: {moved[1] / moved[0]:.2f}x)")

    dsizes = [int(s) for s in args.decode_sizes.split(",") if s]
    for n in sorted({args.n} | set(dsizes), reverse=True):
        gen = torch.Generator(device=dev)
        g16 = []
        for j in range(3):
            gen.manual_seed(j + 1)
            g16.append((torch.randn(n, device=dev, generator=gen) * SIGMA).to(BF16))
        if n == args.n:
            rows = (("threshold", lambda c: c.ThresholdCompressor(THR), ResidualMemory, (12 * n, 28 * n)),
                    ("threshold -m", lambda c: c.ThresholdCompressor(THR), NoneMemory, (4 * n, 20 * n)),
                    ("randomk", lambda c: c.RandomKCompressor(RATIO), ResidualMemory, (12 * n, 28 * n)))
            for row, make, memory, moved in rows:
                parents = argparse.Namespace(ThresholdCompressor=ThresholdCompressor, RandomKCompressor=RandomKCompressor)
                fns = [Step(g16, Allgather(make(sparse_bf16), memory(), 1), cast=False),
                       Step(g16, Allgather(make(parents), memory(), 1), cast=True)]
                report(n, row, time_rows(fns, args), moved)
                del fns
                torch.cuda.empty_cache()
        if n in dsizes:
            buf, cap, counts_dev, counts = padded([g.float() for g in g16], n, dev)
            total = sum(counts)
            fns = [lambda i: ops.sparse_aggregate_padded(buf, cap, counts_dev, W, n, W),
                   lambda i: ops.f32_to_bf16(ops.sparse_aggregate(buf, buf[cap:].view(torch.int32), 2 * cap, counts, W,
                                                                  n, W))]
            # bf16: indices once for the boundaries, entries once, 2 n out.  cast: 4 n fill, per entry 8 read +
            # 8 out read-modify-write + 4 tag, the divide's 4 idx + 4 tag + 8, then 4 n + 2 n to narrow
            report(n, f"decode ({total} entries)", time_rows(fns, args), (2 * n + 12 * total, 10 * n + 36 * total))
            del buf, fns
        del g16
        torch.cuda.empty_cache()
    text = "\n".join(lines + verdicts) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
