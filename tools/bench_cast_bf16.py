"""Natural compression (both flavours), fp16 and one-bit on a bfloat16 gradient against today's
workaround and against the f32 step alone, in one process (no subprocesses), timed with device
events.  Per codec:

  step      the fused world-1 step             bf16: ops.cast_step_w1(g) / ops.onebit_step_w1(g)
                                               cast: the same on g.float(), then .to(bfloat16)
                                               f32 : the same on g32
            one-bit only                       f32 unfused: the f32 class's step as it was (encode,
                                               decode, rank-ordered sum, divide) on g32
  compress  the payload alone                  bf16: ops.*_compress(g) / ops.onebit_encode_grad(g)
                                               cast: the same on g.float()
                                               f32 : the same on g32
  decode    W = 8 rank-major payloads,         bf16: the one-pass decode with out_dtype=bfloat16
            decoded, summed and averaged       cast: the one-pass f32 decode, then .to(bfloat16)

Bytes per element are counted from the launches' arguments, not measured.  Two
inputs: one tensor of 2^26 elements, and the 161 tensors of ResNet-50, each its own tensor and its own
call as these per-tensor codecs are used (a "call" of that input is the whole set, so it is bound by
the launches, not by memory).  Each input has three rotated gradients, as bench.py rotates its
buffers, and every row is warmed up before it is timed.  The variants of a row group alternate in
rounds of --steps calls; each row reports the median, fastest and slowest round in microseconds per
call, the bytes moved and the share of the 8 TB/s peak that is.

--ab-lib PATH adds, per input, an A/B of the f32 natural encode and natural world-1 step between this
build and a build of the parent commit's library at PATH (grace_amd._lib.use), alternating in rounds.

    python tools/bench_cast_bf16.py [--inputs 67108864,resnet50] [--rounds R] [--steps S] [--out FILE]
                                    [--ab-lib PATH]
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
BF16 = torch.bfloat16
NAMES = ("bf16", "cast", "f32", "f32 unfused")
MODE = {"natural": 0, "cnat": 1, "fp16": 3}
# bytes per element: (bf16, cast, f32[, f32 unfused])
BYTES = {("natural", "step"): (4, 20, 8), ("cnat", "step"): (4, 20, 8), ("fp16", "step"): (4, 20, 8),
         ("onebit", "step"): (6, 24, 12, 30),
         ("natural", "compress"): (3, 11, 5), ("cnat", "compress"): (3, 11, 5), ("fp16", "compress"): (4, 12, 6),
         ("onebit", "compress"): (3, 15, 9),
         ("natural", "decode"): (W + 2, W + 10), ("cnat", "decode"): (W + 2, W + 10),
         ("fp16", "decode"): (2 * W + 2, 2 * W + 10), ("onebit", "decode"): (W + 2, W + 10)}


def resnet50_sizes():
    import bench
    sizes = []
    for s in bench.resnet50_shapes():
        k = 1
        for d in s:
            k *= d
        sizes.append(k)
    return sizes


def compress(codec, g, seed):
    if codec == "natural":
        return ops.natural_compress(g, seed=seed)
    if codec == "cnat":
        return ops.cnat_compress(g, seed=seed)
    if codec == "fp16":
        return ops.fp16_compress(g)
    return ops.onebit_encode_grad(g)


def step(codec, g, seed):
    if codec == "onebit":
        return ops.onebit_step_w1(g)[1]
    return ops.cast_step_w1(g, MODE[codec], seed)


def onebit_unfused(g):
    """grace_amd.dist's OneBitCompressor over Allgather(NoneMemory) at world 1, call by call"""
    mask0, means = ops.onebit_encode_grad(g)
    d = ops.onebit_decode(mask0, means[0:1], means[1:2])
    return ops.div_scalar(ops.sum_rank_order([d]), 1)


def decode(codec, payload, n, out_dtype):
    if codec in ("natural", "cnat"):
        return ops.natural_decompress(payload, n, MODE[codec], world=W, aggregate=True, divisor=float(W),
                                      out_dtype=out_dtype)
    if codec == "fp16":
        return ops.fp16_decompress_aggregate(payload, n, W, divisor=float(W), out_dtype=out_dtype)
    return ops.onebit_decode_aggregate(payload[0], payload[1], payload[2], W, n, divisor=float(W), out_dtype=out_dtype)


def payloads(codec, g16):
    """per tensor: W rank-major payloads (the three gradients in turn, different seeds)"""
    out = []
    for t in range(len(g16[0])):
        ps = [compress(codec, g16[w % 3][t], 100 + w) for w in range(W)]
        if codec == "onebit":
            out.append((torch.cat([p[0] for p in ps]), torch.cat([p[1][0:1] for p in ps]),
                        torch.cat([p[1][1:2] for p in ps])))
        else:
            out.append(torch.cat(ps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default=f"{1 << 26},resnet50")
    ap.add_argument("--codecs", default="natural,cnat,fp16,onebit")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100, help="calls per round (a tenth of it for the tensor set)")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default="")
    ap.add_argument("--ab-lib", default="", help="a build of the parent commit's library to A/B the f32 natural "
                                                 "encode and step against")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(dev)}: {args.rounds} rounds per row, us per call (median, min, max of the "
             f"rounds); bytes counted, share of {PEAK / 1e12:.0f} TB/s; decode rows: W = {W}",
             f"{'input':>10} {'row':<30}{'B/elem':>7}{'median us':>11}{'min':>10}{'max':>10}{'MB moved':>10}{'of peak':>9}"]
    ratios = []
    for inp in args.inputs.split(","):
        sizes = resnet50_sizes() if inp == "resnet50" else [int(inp)]
        steps = max(1, args.steps // 10) if inp == "resnet50" else args.steps
        n = sum(sizes)
        lines.append(f"# {inp}: {len(sizes)} tensor(s), {n} elements, {steps} calls per round")
        gen = torch.Generator(device=dev)
        g16, g32 = [], []
        for j in range(3):
            gen.manual_seed(j + 1)
            g16.append([(torch.randn(k, device=dev, generator=gen) * 0.01).to(BF16) for k in sizes])
            g32.append([t.float() for t in g16[-1]])
        T = range(len(sizes))
        for codec in args.codecs.split(","):
            pay = payloads(codec, g16)
            rows = {
                (codec, "step"): [lambda i: [step(codec, g16[i % 3][t], i) for t in T],
                                  lambda i: [step(codec, g16[i % 3][t].float(), i).to(BF16) for t in T],
                                  lambda i: [step(codec, g32[i % 3][t], i) for t in T]],
                (codec, "compress"): [lambda i: [compress(codec, g16[i % 3][t], i) for t in T],
                                      lambda i: [compress(codec, g16[i % 3][t].float(), i) for t in T],
                                      lambda i: [compress(codec, g32[i % 3][t], i) for t in T]],
                (codec, "decode"): [lambda i: [decode(codec, pay[t], sizes[t], BF16) for t in T],
                                    lambda i: [decode(codec, pay[t], sizes[t], torch.float32).to(BF16) for t in T]],
            }
            if codec == "onebit":
                rows[(codec, "step")].append(lambda i: [onebit_unfused(g32[i % 3][t]) for t in T])
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
                        for i in range(steps):
                            f(i)
                        e1.record()
                        e1.synchronize()
                        us[v].append(e0.elapsed_time(e1) / steps * 1e3)
                med = [statistics.median(u) for u in us]
                for v in range(len(fns)):
                    moved = BYTES[key][v] * n
                    lines.append(f"{inp:>10} {key[0] + ' ' + key[1] + ' ' + NAMES[v]:<30}{BYTES[key][v]:>7}{med[v]:>11.1f}"
                                 f"{min(us[v]):>10.1f}{max(us[v]):>10.1f}{moved / 1e6:>10.1f}"
                                 f"{moved / (med[v] * 1e-6) / PEAK:>9.1%}")
                ratios.append(f"{inp}: {key[0]} {key[1]}: cast / bf16 = {med[1] / med[0]:.2f}x (fastest cast round "
                              f"{min(us[1]):.1f} us, slowest bf16 round {max(us[0]):.1f} us: "
                              f"{'apart' if min(us[1]) > max(us[0]) else 'OVERLAP'})" +
                              (f", f32 / bf16 = {med[2] / med[0]:.2f}x" if len(fns) >= 3 else ""))
            del pay, rows
        if args.ab_lib:
            # the two f32 kernels whose instruction text differs from the parent commit's (natural_code's
            # exponent add: one opcode per element), this build against a build of the parent, alternating
            from grace_amd import _lib
            ab = {"natural compress f32": lambda i: [ops.natural_compress(g32[i % 3][t], seed=i) for t in T],
                  "natural step f32": lambda i: [ops.cast_step_w1(g32[i % 3][t], 0, i) for t in T]}
            for row, f in ab.items():
                us = {"this build": [], "parent build": []}
                for _ in range(args.rounds + 1):        # the first round of each build warms it up
                    for build, path in (("this build", _lib.LIB_PATH), ("parent build", args.ab_lib)):
                        _lib.use(path)
                        f(0)
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(steps):
                            f(i)
                        e1.record()
                        e1.synchronize()
                        us[build].append(e0.elapsed_time(e1) / steps * 1e3)
                for build, u in us.items():
                    u = u[1:]
                    lines.append(f"{inp:>10} {'A/B ' + row + ', ' + build:<44}{statistics.median(u):>11.1f}"
                                 f"{min(u):>10.1f}{max(u):>10.1f}")
            _lib.use(_lib.LIB_PATH)
        del g16, g32
        torch.cuda.empty_cache()
    text = "\n".join(lines + ratios) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
