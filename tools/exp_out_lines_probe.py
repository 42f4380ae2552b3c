"""Ceiling of a line-skipping dense output for the world-1 top-k residual step: the
main pass's streaming skeleton (grace_topk_stream_probe) with `out` stored in full (sparse = 0) or
only in a hashed share of its 128-B / 64-B / 32-B lines (sparse = 2 / 3 / 4: 0.52 / 0.31 / 0.17 of
the lines, the shares a CPU replay of the bench's sequence gave for "dirty in this step or the
previous one").  One process, the bench's sequence (3 names, 2^26 elements, ratio 0.01); every
variant runs on the SAME buffer sets (placed by ops.pick_pair, as the engine places its own), the
variants alternate launch by launch, a real step runs before every probe launch, and the launches
are timed with the library's dispatch-packet events like the main pass.  The dense variant is in
the rotation twice (as "dense" and "dense_b"): the gap between their medians is the spread a
variant has to beat.

Usage: python tools/exp_out_lines_probe.py [--numel N] [--rounds R] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grace_amd import _lib, ops  # noqa: E402
from grace_amd.dist.communicator.allgather import Allgather  # noqa: E402
from grace_amd.dist.compressor.topk import TopKCompressor  # noqa: E402
from grace_amd.dist.memory.residual import ResidualMemory  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--numel", type=int, default=64 * 1024 * 1024)
ap.add_argument("--rounds", type=int, default=16)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()

n, dev = args.numel, torch.device("cuda", 0)
comm = Allgather(TopKCompressor(0.01), ResidualMemory(), 1)
gen = torch.Generator(device=dev)
grads = []
for j in range(3):
    gen.manual_seed(j + 1)
    grads.append(torch.randn(n, device=dev, generator=gen))


def step(i):
    comm.step(grads[i % 3], f"bucket{i % 3}")


for i in range(9):
    step(i)

bufs = []
for _ in range(args.sets):
    g = torch.zeros(n, dtype=torch.float32, device=dev)
    r, o = ops.pick_pair(g)[:2] if ops.PLACE_PROBE and n >= ops.PLACE_MIN_N else (torch.zeros_like(g),
                                                                                    torch.zeros_like(g))
    bufs.append((g, r, o))
ws = torch.zeros(int(_lib.query("grace_topk_stream_probe_workspace_bytes", n)), dtype=torch.uint8, device=dev)

variants = [("dense", 0), ("lines128_0.52", 2), ("lines64_0.31", 3), ("dense_b", 0), ("lines32_0.17", 4),
            ("no_out", 1)]
us = {name: [] for name, _ in variants}
it = 0
for rnd in range(args.rounds + 1):
    for s in range(args.sets):
        g, r, o = bufs[s]
        # the variants in a rotated order per (round, set), so that none always follows the same one
        for v in range(len(variants)):
            name, mode = variants[(v + rnd + s) % len(variants)]
            step(it)
            it += 1
            ops.timer_enable(True)
            _lib.call("grace_topk_stream_probe", g.data_ptr(), r.data_ptr(), o.data_ptr(), n, mode, ws.data_ptr(),
                      ws.numel(), ops._stream())
            ms, cnt = ops.timer_collect()
            ops.timer_enable(False)
            if rnd >= 1 and cnt == 1:
                us[name].append(ms * 1e3)

res = {"numel": n, "sets": args.sets, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
       "launches_per_variant": {k: len(v) for k, v in us.items()},
       "median_us": {k: round(statistics.median(v), 2) for k, v in us.items() if v},
       "min_us": {k: round(min(v), 2) for k, v in us.items() if v},
       "p25_p75_us": {k: [round(x, 2) for x in (statistics.quantiles(v, n=4)[0], statistics.quantiles(v, n=4)[2])]
                      for k, v in us.items() if len(v) >= 4},
       # per buffer set: the placement differs between sets, the variants share it within one
       "median_us_per_set": {k: [round(statistics.median(v[s::args.sets]), 2) for s in range(args.sets)]
                             for k, v in us.items() if len(v) >= args.sets}}
m = res["median_us"]
res["dense_spread_us"] = round(abs(m["dense"] - m["dense_b"]), 2)
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
