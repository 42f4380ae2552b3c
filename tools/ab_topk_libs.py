"""In-process A/B of builds of libgrace_hip on the bench's own sequence: Allgather(TopK 1 %,
ResidualMemory, 1).step over 3 names of `--numel` f32 elements.  Every build runs on the SAME
gradient, residual and output buffers and line maps (one communicator; only the loaded library is
switched), the builds alternate in blocks of `--block` steps, `--blocks` blocks per build; the
first steps after every switch run untimed.  Per block: ms per step (two stream events around the
block) and the event-timed topk_main average (the library's dispatch-packet timer).

A variant is `NAME=PATH` or `NAME=PATH:GRID`, GRID being passed to grace_topk_main_grid_limit (builds
that have it); the first variant is the base.  A variant counts as faster only if its ranges are
disjoint from the base's on both figures: its slowest block faster than the base's fastest.

Usage: python tools/ab_topk_libs.py base=LIB_A new=LIB_B [new1024=LIB_B:1024 ...] [--numel N] [--out FILE.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grace_amd import _lib, ops  # noqa: E402
from grace_amd.dist.communicator.allgather import Allgather  # noqa: E402
from grace_amd.dist.compressor.topk import TopKCompressor  # noqa: E402
from grace_amd.dist.memory.residual import ResidualMemory  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("variants", nargs="+")
ap.add_argument("--numel", type=int, default=64 * 1024 * 1024)
ap.add_argument("--block", type=int, default=21)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()

variants = []
for v in args.variants:
    name, spec = v.split("=", 1)
    path, _, grid = spec.partition(":")
    variants.append((name, path, int(grid or 0)))


def switch(path, grid):
    lib = _lib.use(path)
    if hasattr(lib, "grace_topk_main_grid_limit"):
        lib.grace_topk_main_grid_limit(grid)
    elif grid:
        sys.exit(f"{path} has no grace_topk_main_grid_limit")


n, dev, names = args.numel, torch.device("cuda", 0), 3
switch(variants[0][1], variants[0][2])
if n < ops.PLACE_MIN_N:
    # smaller buckets keep their output buffer (and its line map) for this run too, as in
    # tools/ab_out_lines.py, with plain allocations in place of the probed pair
    ops.PLACE_MIN_N = n
    ops.pick_pair = lambda g, *a: (torch.empty_like(g), torch.empty_like(g), [])
comm = Allgather(TopKCompressor(0.01), ResidualMemory(), 1)
gen = torch.Generator(device=dev)
grads = []
for j in range(names):
    gen.manual_seed(j + 1)
    grads.append(torch.randn(n, device=dev, generator=gen))
it = 0


def step():
    global it
    comm.step(grads[it % names], f"bucket{it % names}")
    it += 1


for _ in range(3 * names):
    step()
rec = comm.compressor._recycler
blocks = {name: [] for name, _, _ in variants}
for b in range(args.blocks):
    for name, path, grid in variants:
        torch.cuda.synchronize()
        switch(path, grid)
        for _ in range(2 * names):
            step()
        torch.cuda.synchronize()
        d0 = rec.dense_hits
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.timer_enable(True)
        e0.record()
        for _ in range(args.block):
            step()
        e1.record()
        e1.synchronize()
        main_ms, launches = ops.timer_collect()
        ops.timer_enable(False)
        assert rec.dense_hits - d0 == args.block, "a step of the block did not get its kept buffer back"
        blocks[name].append({"ms_per_step": round(e0.elapsed_time(e1) / args.block, 4),
                             "topk_main_us": round(main_ms * 1e3 / max(launches, 1), 2)})
torch.cuda.synchronize()

res = {"numel": n, "names": names, "block_steps": args.block, "device": torch.cuda.get_device_name(0),
       "variants": {name: {"lib": os.path.basename(path), "grid_limit": grid} for name, path, grid in variants},
       "blocks": blocks, "ranges": {}}
base = variants[0][0]
for key in ("ms_per_step", "topk_main_us"):
    b = [x[key] for x in blocks[base]]
    res["ranges"][key] = {}
    for name, _, _ in variants:
        v = [x[key] for x in blocks[name]]
        res["ranges"][key][name] = {"min": min(v), "max": max(v), "disjoint_faster_than_base": max(v) < min(b),
                                    "slower_than_base": min(v) > max(b)}
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
