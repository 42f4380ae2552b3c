"""The world-1 top-k 1 % + residual step on a bfloat16 gradient, three ways, in one process:

  (a) f32   the f32 step on g.float() prepared outside the timed region      16 B per element
  (b) cast  today's workaround, all timed: g.float(), the f32 step, .to(bf16) 28 B per element
  (a') f32op the same f32 step called as row (c) is, for a like-for-like pair  16 B per element
  (c) bf16  the bf16 step (ops.topk_residual_step: grace_topk_residual_step_bf16) 12 B per element

n = 2^26, k = 1 %, ResidualMemory, steady state.  The buffer-placement probe is off
(GRACE_PLACE_PROBE=0), so that the f32 rows do not depend on which allocations they drew.  The
variants alternate in rounds of --steps steps timed with device events; each row reports the median,
the fastest and the slowest round (the spread) in ms per step, and the main pass's own event time.
Bytes per element are counted from the shapes, not measured.  Rows (a) and (b) go through Allgather(TopKCompressor, ResidualMemory).step;
rows (a') and (c) call ops.topk_residual_step itself, with a new result tensor per step and the
residual and its sample carry kept as that step keeps them, so (a') against (c) differs in the
element type only.  With a library that has no bf16 entry
points (an older build) row (c) is skipped and (a), (b) still run.

    python tools/bench_topk_bf16.py [--n N] [--rounds R] [--steps S] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

os.environ["GRACE_PLACE_PROBE"] = "0"

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grace_amd import _lib, ops  # noqa: E402
from grace_amd.dist.communicator.allgather import Allgather  # noqa: E402
from grace_amd.dist.compressor.topk import TopKCompressor  # noqa: E402
from grace_amd.dist.memory.residual import ResidualMemory  # noqa: E402

BYTES = {"f32": 16, "cast": 28, "f32op": 16, "bf16": 12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--ratio", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    have_bf16 = "grace_topk_residual_step_bf16" in _lib.SIGNATURES
    k = ops.ratio_k(n, args.ratio)
    gen = torch.Generator(device=dev)
    grads = []
    for j in range(3):   # three rotated gradients, one name: the residual carries over
        gen.manual_seed(j + 1)
        grads.append(torch.randn(n, device=dev, generator=gen).to(torch.bfloat16))
    grads32 = [g.float() for g in grads]
    comms = {m: Allgather(TopKCompressor(args.ratio), ResidualMemory(), 1) for m in ("f32", "cast")}
    size = ops.topk_carry_size(n, k)
    state = {m: {"steps": 0, "res": torch.empty(n, dtype=torch.float32, device=dev),
                 "carry": torch.empty(size, dtype=torch.float32, device=dev) if size else None}
             for m in ("f32op", "bf16")}

    def step(m, i):
        if m == "f32":
            return comms[m].step(grads32[i % 3], "w")
        if m == "cast":
            return comms[m].step(grads[i % 3].float(), "w").to(torch.bfloat16)
        g, st = (grads32 if m == "f32op" else grads)[i % 3], state[m]
        out = torch.empty_like(g)
        has = st["steps"] > 0
        ops.topk_residual_step(g, st["res"], has, 1.0, 1.0, k, out=out, carry=st["carry"], carry_valid=has)
        st["steps"] += 1
        return out

    rows = [m for m in BYTES if m != "bf16" or have_bf16]
    for i in range(args.warmup):
        for m in rows:
            step(m, i)
    ms = {m: [] for m in rows}
    main_us = {m: [] for m in rows}
    for _ in range(args.rounds):
        for m in rows:
            torch.cuda.synchronize()
            ops.timer_enable(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                step(m, i)
            e1.record()
            e1.synchronize()
            t, cnt = ops.timer_collect()
            ops.timer_enable(False)
            ms[m].append(e0.elapsed_time(e1) / args.steps)
            main_us[m].append(t / max(cnt, 1) * 1e3)
    result = {"n": n, "ratio": args.ratio, "rounds": args.rounds, "steps_per_round": args.steps,
              "device": torch.cuda.get_device_name(dev), "bf16_entry_points": have_bf16, "rows": {}}
    print(f"n = {n}, k = {ops.ratio_k(n, args.ratio)}, {args.rounds} rounds of {args.steps} steps, "
          f"{result['device']}")
    print(f"{'row':<7}{'B/elem':>7}{'ms/step median':>16}{'min':>9}{'max':>9}{'main pass us':>14}")
    for m in rows:
        v = ms[m]
        r = {"bytes_per_element": BYTES[m], "ms_per_step_median": round(statistics.median(v), 4),
             "ms_per_step_min": round(min(v), 4), "ms_per_step_max": round(max(v), 4),
             "main_pass_us_median": round(statistics.median(main_us[m]), 1)}
        result["rows"][m] = r
        print(f"{m:<7}{BYTES[m]:>7}{r['ms_per_step_median']:>16.4f}{r['ms_per_step_min']:>9.4f}"
              f"{r['ms_per_step_max']:>9.4f}{r['main_pass_us_median']:>14.1f}")
    if not have_bf16:
        print("bf16   skipped: this library has no bf16 top-k entry points")
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
