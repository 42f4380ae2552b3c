"""Adaptive quantisation (grace_amd/csrc/adaq.hip) at 2^26 elements, f32 and bf16,
ratio 0.01 and 0.1, in one process, timed with device events, on a normal gradient of scale 1e-3:

  compress   ops.adaq_compress                    the fixed-size payload; no host read
  step       ops.adaq_step_w1                     the world-1 step, dense result in g's dtype
  decode     ops.adaq_decode_aggregate, W = 8     eight payloads, averaged, result in g's dtype

Beside each row: (a) the row's bytes over 8 TB/s, counted from the launches' arguments, not measured
(compress reads x three times in the select, twice for bf16, once in the count pass and once in the write
pass, and writes the payload; the step writes the result instead; the decode reads W payloads and writes
the result), and the rate those bytes imply; (b) the nearest sparse codec of this library on the same
tensor (topk_compress at the same ratio; threshold_step_w1 with the bound at that quantile;
sparse_aggregate_sorted has another wire, so the decode has no (b)); (c) the eager-PyTorch composition a
user has without the codec: two topk calls on masked magnitudes, mean and index_put_.  The variants of a
row alternate in rounds of --steps calls (a tenth of them for the eager composition); each reports the
median, fastest and slowest round in microseconds per call.

The select alone has no entry point of its own.  --only-compress runs nothing but warm compress calls, so
that a kernel trace of the process (one row a kernel: aq_zero, aq_hist_e, aq_resolve are the select) splits
the time by kernel.

    python tools/bench_adaq.py [--n N] [--rounds R] [--steps S] [--out FILE] [--only-compress]
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grace_amd import ops  # noqa: E402

W = 8
PEAK = 8e12


def eager_select(g, ratio):
    """(indices, values) of the composition: per sign the k largest magnitudes, replaced by their mean"""
    x = g.float().view(-1)
    idx, val = [], []
    for cls in (x > 0, x < 0):
        k = math.ceil(int(cls.sum()) * ratio)
        top = torch.topk(torch.where(cls, x.abs(), torch.zeros_like(x)), max(k, 1)).indices
        idx.append(top)
        val.append(x[top].mean().expand(top.numel()))
    return torch.cat(idx), torch.cat(val)


def eager_step(g, ratio):
    idx, val = eager_select(g, ratio)
    return torch.zeros(g.numel(), device=g.device).index_put_((idx,), val).to(g.dtype)


def eager_decode(parts, n, dtype):
    acc = torch.zeros(n, device=parts[0][0].device)
    for idx, val in parts:
        acc = acc + torch.zeros_like(acc).index_put_((idx,), val)
    return (acc / W).to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--only-compress", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    emit(f"{torch.cuda.get_device_name(dev)}: n = {n}, {args.rounds} rounds of {args.steps} calls per row, us per call "
         f"(median, min, max of the rounds); bytes counted; (a) = bytes / {PEAK / 1e12:.0f} TB/s; decode: W = {W}")
    emit(f"{'row':<44}{'B/elem':>7}{'(a) us':>9}{'median us':>13}{'min':>13}{'max':>13}{'TB/s':>7}{'of peak':>9}")
    ratios = []
    gen = torch.Generator(device=dev).manual_seed(1)
    base = [torch.randn(n, device=dev, generator=gen) * 1e-3 for _ in range(3)]
    for dtype, name, sz in ((torch.float32, "f32", 4), (torch.bfloat16, "bf16", 2)):
        g = [t.to(dtype) for t in base]
        for ratio in (0.01, 0.1):
            if args.only_compress:
                for i in range(args.steps):
                    ops.adaq_compress(g[i % 3], ratio)
                torch.cuda.synchronize()
                continue
            total = ops.adaq_payload_bytes(n, ratio)
            wire = torch.cat([ops.adaq_compress(g[w % 3], ratio) for w in range(W)])
            parts = [eager_select(g[w % 3], ratio) for w in range(W)]
            k = ops.ratio_k(n, ratio)
            thr = float(g[0].float().abs().view(-1)[:1 << 20].kthvalue(int((1 << 20) * (1 - ratio))).values)
            reads = (3 if sz == 4 else 2) + 2                      # select, count pass, last pass
            rows = {
                "compress": ((reads * sz * n + total) / n, [
                    lambda i: ops.adaq_compress(g[i % 3], ratio), lambda i: ops.topk_compress(g[i % 3], k),
                    lambda i: eager_select(g[i % 3], ratio)]),
                "step": ((reads * sz * n + sz * n) / n, [
                    lambda i: ops.adaq_step_w1(g[i % 3], ratio),
                    lambda i: ops.threshold_step_w1(g[i % 3], None, 0, 1.0, 1.0, thr),
                    lambda i: eager_step(g[i % 3], ratio)]),
                "decode": ((W * total + sz * n) / n, [
                    lambda i: ops.adaq_decode_aggregate(wire, W, n, ratio, divisor=float(W), out_dtype=dtype), None,
                    lambda i: eager_decode(parts, n, dtype)]),
            }
            emit(f"{name} ratio {ratio}: the payload is {total} bytes, {total / (4 * n):.2%} of the float32 bytes")
            for row, (bpe, fns) in rows.items():
                steps = [args.steps, args.steps, max(1, args.steps // 10)]
                us = [[] for _ in fns]
                for f in fns:
                    for i in range(args.warmup if f else 0):
                        f(i)
                for _ in range(args.rounds):
                    for v, f in enumerate(fns):      # the variants of one row alternate
                        if f is None:
                            continue
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(steps[v]):
                            f(i)
                        e1.record()
                        e1.synchronize()
                        us[v].append(e0.elapsed_time(e1) / steps[v] * 1e3)
                med = [statistics.median(u) if u else None for u in us]
                tag = f"{name} {ratio} {row}"
                for v, what in enumerate(("adaq", "(b) topk" if row == "compress" else "(b) threshold", "(c) eager")):
                    if med[v] is None:
                        continue
                    b = bpe if v == 0 else None
                    floor = f"{b * n / PEAK * 1e6:>9.1f}" if b else f"{'':>9}"
                    rate = f"{b * n / (med[v] * 1e-6) / 1e12:>7.2f}{b * n / (med[v] * 1e-6) / PEAK:>9.1%}" if b else ""
                    emit(f"{tag + ' ' + what:<44}{(f'{b:.2f}' if b else ''):>7}{floor}{med[v]:>13.1f}"
                         f"{min(us[v]):>13.1f}{max(us[v]):>13.1f}{rate}")
                ratios.append(f"{tag}: " + (f"time / (b)'s = {med[0] / med[1]:.2f}x, " if med[1] else "") +
                              f"eager / adaq = {med[2] / med[0]:.1f}x")
            del wire, parts
            torch.cuda.empty_cache()
    print("\n".join(ratios), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines + ratios) + "\n")


if __name__ == "__main__":
    main()
