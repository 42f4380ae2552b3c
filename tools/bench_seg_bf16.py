"""The world-1 segmented per-tensor top-k 1 % + residual step (SegmentedTopK) over ResNet-50's 161
gradient tensors, for a bfloat16 gradient bucket, three ways in one process:

  (a) f32   the f32 step in place on an f32 bucket (the gradient cast outside the timed region)  16 B per element
  (b) cast  what a bf16 user had to do, all timed: bucket.float(), the f32 step in place on that
            copy, and the cast back down into the bf16 bucket                                   28 B per element
  (c) bf16  the bf16 step in place on the bf16 bucket (grace_amd.segmented_bf16.SegmentedTopK)   12 B per element

Each row owns its engine, its residual and --steps buckets.  Before every round the buckets are
refilled (untimed) from three seeded gradients in rotation, the same ones for every row; inside a
round step i runs in place on bucket i, as harness.step_segmented does on a bucket a backward pass
has just written, so every timed step sees a fresh gradient and the residual of the steps before it.
--reuse-bucket steps ONE bucket per row over and over on its own result instead (refilled only
before each round), as bench.py's ddp_segmented does; DESIGN.md §9 says what that does to rows (b)
and (c), whose result is rounded to bf16.
The rows alternate in rounds of --steps steps timed with device events; each row reports the median,
the fastest and the slowest round (the spread) in us per step, and the main pass's own event time.
After a row's last round the tool reads the status word of every large segment's workspace and
reports how many took the exact fallback in that last step, and their sizes.
Bytes per element are counted from the shapes, not measured.  With a library that has no bf16
segmented entry point (an older tree: --tree DIR) row (c) is skipped and (a), (b) still run.

    python tools/bench_seg_bf16.py [--tree DIR] [--rounds R] [--steps S] [--reuse-bucket] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

os.environ["GRACE_PLACE_PROBE"] = "0"

import numpy as np  # noqa: E402
import torch  # noqa: E402

BYTES = {"f32": 16, "cast": 28, "bf16": 12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose grace_amd (and built library) is measured")
    ap.add_argument("--ratio", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--reuse-bucket", action="store_true", help="one bucket per row, stepped on its own result")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import bench
    from grace_amd import _lib, ops
    from grace_amd.dist.segmented import SegmentedTopK
    dev = torch.device("cuda", 0)
    sizes = [int(np.prod(s)) for s in bench.resnet50_shapes()]
    n = sum(sizes)
    have_bf16 = "grace_topk_segmented_step_bf16" in _lib.SIGNATURES
    gen = torch.Generator(device=dev)
    grads = []
    for j in range(3):
        gen.manual_seed(j + 1)
        grads.append((torch.randn(n, device=dev, generator=gen) * 0.01).to(torch.bfloat16))
    grads32 = [g.float() for g in grads]
    rows = [m for m in BYTES if m != "bf16" or have_bf16]
    eng = {m: SegmentedTopK(args.ratio) for m in rows}
    if have_bf16:   # the subclass that takes bf16; rows (a) and (b) stay on grace_amd.dist's class
        from grace_amd.segmented_bf16 import SegmentedTopK as SegmentedTopKBf16
        eng["bf16"] = SegmentedTopKBf16(args.ratio)
    buf = {m: [torch.empty(n, dtype=torch.float32 if m == "f32" else torch.bfloat16, device=dev)
               for _ in range(1 if args.reuse_bucket else args.steps)] for m in rows}

    def refill(m, j):
        for i, b in enumerate(buf[m]):
            b.copy_((grads32 if m == "f32" else grads)[(j + i) % 3])

    def step(m, i):
        b = buf[m][i % len(buf[m])]
        if m == "cast":
            t = b.float()
            eng[m].step(t, sizes, out=t)
            b.copy_(t)
        else:
            eng[m].step(b, sizes, out=b)

    for m in rows:
        refill(m, 0)
        for i in range(min(args.warmup, args.steps)):
            step(m, i)

    def fallbacks(m):
        """Sizes of the large segments whose last step ended in the exact fallback (ctl status 1)."""
        T = eng[m].tables(sizes, dev, True, True)    # (the bf16 step shares this entry's workspace)
        nl = T["n_large"]
        status = T["ws"].view(torch.int32)[T["ws_off"][:nl] // 4 + 3].tolist()
        large = T["large"][:nl].tolist()
        return nl, [sizes[large[li]] for li in range(nl) if status[li] == 1]

    us = {m: [] for m in rows}
    main_us = {m: [] for m in rows}
    for rnd in range(args.rounds):
        for m in rows:
            refill(m, rnd)
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
            us[m].append(e0.elapsed_time(e1) / args.steps * 1e3)
            main_us[m].append(t / max(cnt, 1) * 1e3)
    result = {"tensors": len(sizes), "numel": n, "ratio": args.ratio, "rounds": args.rounds,
              "steps_per_round": args.steps, "device": torch.cuda.get_device_name(dev),
              "bf16_entry_point": have_bf16, "reuse_bucket": args.reuse_bucket, "rows": {}}
    print(f"{len(sizes)} tensors, {n} elements, ratio {args.ratio}, {args.rounds} rounds of {args.steps} steps, "
          f"{result['device']}" + (", one bucket per row stepped on its own result" if args.reuse_bucket else ""))
    print(f"{'row':<7}{'B/elem':>7}{'us/step median':>16}{'min':>9}{'max':>9}{'main pass us':>14}")
    for m in rows:
        v = us[m]
        r = {"bytes_per_element": BYTES[m], "us_per_step_median": round(statistics.median(v), 1),
             "us_per_step_min": round(min(v), 1), "us_per_step_max": round(max(v), 1),
             "main_pass_us_median": round(statistics.median(main_us[m]), 1)}
        nl, fb = fallbacks(m)
        r["large_segments"], r["exact_fallback_sizes_last_step"] = nl, fb
        result["rows"][m] = r
        print(f"{m:<7}{BYTES[m]:>7}{r['us_per_step_median']:>16.1f}{r['us_per_step_min']:>9.1f}"
              f"{r['us_per_step_max']:>9.1f}{r['main_pass_us_median']:>14.1f}")
    for m in rows:
        fb = result["rows"][m]["exact_fallback_sizes_last_step"]
        print(f"{m:<7}exact fallback in the last step: {len(fb)} of {result['rows'][m]['large_segments']} large segments"
              + (f", sizes {sorted(fb, reverse=True)}" if fb else ""))
    if not have_bf16:
        print("bf16   skipped: this library has no bf16 segmented entry point")
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
