"""The world-1 EF-signSGD and signSGD steps on a bfloat16 gradient against today's workaround, in one
process (no subprocesses), timed with device events:

  ef_bf16    Allgather(sign_bf16.EFSignSGDCompressor, EFSignSGDMemory, 1).step(g)        18 B per element
  ef_cast    g.float() -> the f32 Allgather(EFSignSGDCompressor, EFSignSGDMemory, 1).step
             -> .to(bfloat16)                                                           71 B per element
  sign_bf16  Allgather(sign_bf16.SignSGDCompressor, NoneMemory, 1).step(g)                4 B per element
  sign_cast  g.float() -> the f32 signSGD step -> .to(bfloat16)                          20 B per element

Bytes per element are counted from the launches' arguments, not measured.
Each size (2^20 and 2^26 elements by default) has three rotated gradients of one name, as bench.py
rotates its buffers, and is warmed up before it is timed; the two variants of a pair alternate in
rounds of --steps steps.  Each row reports the median, fastest and slowest round in microseconds per
step, the bytes moved, and the share of the 8 TB/s peak that is.

    python tools/bench_sign_bf16.py [--sizes 1048576,67108864] [--rounds R] [--steps S] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grace_amd import sign_bf16  # noqa: E402
from grace_amd.dist.communicator.allgather import Allgather  # noqa: E402
from grace_amd.dist.compressor.efsignsgd import EFSignSGDCompressor  # noqa: E402
from grace_amd.dist.compressor.signsgd import SignSGDCompressor  # noqa: E402
from grace_amd.dist.memory.efsignsgd import EFSignSGDMemory  # noqa: E402
from grace_amd.dist.memory.none import NoneMemory  # noqa: E402

BYTES = {"ef_bf16": 18, "ef_cast": 71, "sign_bf16": 4, "sign_cast": 20}
PEAK = 8e12
LR = 0.1
BF16 = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"{1 << 20},{1 << 26}")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(dev)}: {args.rounds} rounds of {args.steps} steps per row, "
             f"us per step (median, min, max of the rounds); bytes counted, share of {PEAK / 1e12:.0f} TB/s",
             f"{'n':>10} {'row':<10}{'B/elem':>7}{'median us':>11}{'min':>10}{'max':>10}{'MB moved':>10}{'of peak':>9}"]
    ratios = []
    for n in (int(s) for s in args.sizes.split(",")):
        gen = torch.Generator(device=dev)
        grads = []
        for j in range(3):
            gen.manual_seed(j + 1)
            grads.append(torch.randn(n, device=dev, generator=gen).to(BF16))
        comms = {"ef_bf16": Allgather(sign_bf16.EFSignSGDCompressor(LR), EFSignSGDMemory(LR), 1),
                 "ef_cast": Allgather(EFSignSGDCompressor(LR), EFSignSGDMemory(LR), 1),
                 "sign_bf16": Allgather(sign_bf16.SignSGDCompressor(), NoneMemory(), 1),
                 "sign_cast": Allgather(SignSGDCompressor(), NoneMemory(), 1)}

        def step(m, i):
            g = grads[i % 3]
            if m.endswith("_cast"):
                return comms[m].step(g.float(), "w").to(BF16)
            return comms[m].step(g, "w")

        for i in range(args.warmup):
            for m in BYTES:
                step(m, i)
        us = {m: [] for m in BYTES}
        for _ in range(args.rounds):
            for m in BYTES:          # ef_bf16, ef_cast, sign_bf16, sign_cast: each pair alternates
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.steps):
                    step(m, i)
                e1.record()
                e1.synchronize()
                us[m].append(e0.elapsed_time(e1) / args.steps * 1e3)
        for m in BYTES:
            med = statistics.median(us[m])
            moved = BYTES[m] * n
            lines.append(f"{n:>10} {m:<10}{BYTES[m]:>7}{med:>11.1f}{min(us[m]):>10.1f}{max(us[m]):>10.1f}"
                         f"{moved / 1e6:>10.1f}{moved / (med * 1e-6) / PEAK:>9.1%}")
        for a, b in (("ef_bf16", "ef_cast"), ("sign_bf16", "sign_cast")):
            ratios.append(f"n = {n}: {b} / {a} = {statistics.median(us[b]) / statistics.median(us[a]):.2f}x")
        del grads, comms
        torch.cuda.empty_cache()
    text = "\n".join(lines + ratios) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
