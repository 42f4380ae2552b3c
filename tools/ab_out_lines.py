"""In-process A/B of the line-skipping dense output (ops.OUT_LINES) on the bench's own
sequence: Allgather(TopK 1 %, ResidualMemory, 1).step over 3 names of `--numel` f32 elements, the
same residual / output buffers throughout (the switch only decides whether the kept buffer's line
map is passed), the switch alternated in blocks of `--block` steps, `--blocks` blocks per mode.
Per block: ms per step (two stream events around the block) and the event-timed topk_main average
(the library's dispatch-packet timer).  The first 3 steps after every switch are run untimed: the
step after switching on writes every line once, and each name has to take that step.

The change counts as a gain only if the ranges do not overlap: the slowest block with the map must
be faster than the fastest block without it.

Usage: python tools/ab_out_lines.py [--numel N] [--block 21] [--blocks 5] [--out FILE.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grace_amd import ops  # noqa: E402
from grace_amd.dist.communicator.allgather import Allgather  # noqa: E402
from grace_amd.dist.compressor.topk import TopKCompressor  # noqa: E402
from grace_amd.dist.memory.residual import ResidualMemory  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--numel", type=int, default=64 * 1024 * 1024)
ap.add_argument("--block", type=int, default=21)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()

n, dev, names = args.numel, torch.device("cuda", 0), 3
if n < ops.PLACE_MIN_N:
    # the compressor keeps an output buffer (and so its line map) only from PLACE_MIN_N elements on;
    # for the question whether smaller buckets should keep theirs too, keep them for this run, with
    # plain allocations in place of the probed pair
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
blocks = {"lines": [], "full": []}
for b in range(2 * args.blocks):
    mode = "lines" if b % 2 == 0 else "full"
    ops.OUT_LINES = mode == "lines"
    for _ in range(2 * names):   # every name takes its first step in this mode (and the one after) untimed
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
    blocks[mode].append({"ms_per_step": round(e0.elapsed_time(e1) / args.block, 4),
                         "topk_main_us": round(main_ms * 1e3 / max(launches, 1), 2)})
ops.OUT_LINES = True
for _ in range(2 * names):
    step()

# the share of the output's 64-B lines the main pass stores in a step: marked now or in the previous step
written = None
ent = rec._hit.get("bucket0")
if ent is not None and ent[6] is not None:
    cur = ent[6][16:].clone()
    step(), step(), step()
    nxt = rec._hit["bucket0"][6][16:]
    both = (cur | nxt).cpu().numpy().view("uint8")
    import numpy as np
    written = {"marked_now": round(float(np.unpackbits(nxt.cpu().numpy().view("uint8")).mean()), 4),
               "written_now_or_previous": round(float(np.unpackbits(both).mean()), 4)}

res = {"numel": n, "names": names, "block_steps": args.block, "device": torch.cuda.get_device_name(0), "blocks": blocks,
       "lines_share": written}
for key in ("ms_per_step", "topk_main_us"):
    lo = [x[key] for x in blocks["lines"]]
    hi = [x[key] for x in blocks["full"]]
    res[key + "_range"] = {"lines": [min(lo), max(lo)], "full": [min(hi), max(hi)],
                           "ranges_disjoint_in_favour_of_lines": max(lo) < min(hi)}
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
