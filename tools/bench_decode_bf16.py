"""The world > 1 sparse decode to a bfloat16 result, three ways, in one process:

  (a) f32   ops.sparse_aggregate_sorted (grace_sparse_aggregate_sorted)              4 B per element
  (b) cast  the f32 aggregate, then ops.f32_to_bf16 (4 written, 4 read, 2 written)  10 B per element
  (c) bf16  ops.sparse_aggregate_sorted(out_dtype=bfloat16): the decode narrows in   2 B per element
            its epilogue (grace_sparse_aggregate_sorted_bf16)

n = 2^26, k = 1 %, W = 8 synthetic payloads grouped by ops.sort_payload on one device, divisor W,
steady state.  Every row also reads the W grouped payloads (6 B per entry: 0.48 B per element at
W = 8, k = 1 %).  Bytes per element are counted from the shapes, not measured.  The rows alternate
in rounds of --steps decodes timed with device events; each row reports the median, the fastest and
the slowest round in microseconds per decode.  The yardstick for (c) is (b).  With --lib an older
build of the library is measured instead; where it has no bf16 decode, row (c) is skipped and (a),
(b) still run.

    python tools/bench_decode_bf16.py [--n N] [--world W] [--rounds R] [--steps S] [--lib SO] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grace_amd import _lib, ops  # noqa: E402

BYTES = {"f32": 4, "cast": 10, "bf16": 2}
BF16 = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--ratio", type=float, default=0.01)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = _lib.use(args.lib) if args.lib else _lib.load()
    have_bf16 = hasattr(lib, "grace_sparse_aggregate_sorted_bf16")
    dev = torch.device("cuda", 0)
    n, world = args.n, args.world
    k = ops.ratio_k(n, args.ratio)
    gen = torch.Generator(device=dev)
    parts = []
    for w in range(world):   # every rank: k distinct indices, normal values, grouped as on the wire
        gen.manual_seed(w + 1)
        buf, vals, idx = ops.new_payload(k, dev)
        idx.copy_(torch.randperm(n, device=dev, generator=gen)[:k])
        vals.copy_(torch.randn(k, device=dev, generator=gen))
        parts.append(ops.sort_payload(buf, k, n))
    gathered = torch.cat(parts)
    del parts
    divisor = float(world)

    def step(m):
        if m == "f32":
            return ops.sparse_aggregate_sorted(gathered, k, world, n, divisor)
        if m == "cast":
            return ops.f32_to_bf16(ops.sparse_aggregate_sorted(gathered, k, world, n, divisor))
        return ops.sparse_aggregate_sorted(gathered, k, world, n, divisor, out_dtype=BF16)

    rows = [m for m in BYTES if m != "bf16" or have_bf16]
    if have_bf16:
        same = torch.equal(step("cast").view(torch.int16), step("bf16").view(torch.int16))
    for _ in range(args.warmup):
        for m in rows:
            step(m)
    us = {m: [] for m in rows}
    for _ in range(args.rounds):
        for m in rows:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(args.steps):
                step(m)
            e1.record()
            e1.synchronize()
            us[m].append(e0.elapsed_time(e1) / args.steps * 1e3)
    payload_b = world * 6 * k / n
    result = {"n": n, "k": k, "world": world, "rounds": args.rounds, "steps_per_round": args.steps,
              "device": torch.cuda.get_device_name(dev), "library": args.lib or _lib.LIB_PATH,
              "bf16_decode": have_bf16, "payload_read_bytes_per_element": round(payload_b, 3), "rows": {}}
    if have_bf16:
        result["bf16_equals_cast_bitwise"] = bool(same)
    print(f"n = {n}, k = {k}, W = {world}, {args.rounds} rounds of {args.steps} decodes, {result['device']}")
    print(f"{'row':<6}{'B/elem':>7}{'+payload':>9}{'us/decode median':>18}{'min':>9}{'max':>9}")
    for m in rows:
        v = us[m]
        r = {"bytes_per_element": BYTES[m], "us_per_decode_median": round(statistics.median(v), 1),
             "us_per_decode_min": round(min(v), 1), "us_per_decode_max": round(max(v), 1)}
        result["rows"][m] = r
        print(f"{m:<6}{BYTES[m]:>7}{payload_b:>9.2f}{r['us_per_decode_median']:>18.1f}{r['us_per_decode_min']:>9.1f}"
              f"{r['us_per_decode_max']:>9.1f}")
    if not have_bf16:
        print("bf16  skipped: this library has no bf16 decode")
    else:
        print(f"bf16 result equals the cast row's bit for bit: {same}")
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
