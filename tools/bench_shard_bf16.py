"""Per-rank device time of the sharded top-k step (BASELINE configs[4]: 2^26 elements, k = 0.1 %,
W = 8) on bfloat16 shards, three ways, without the collective: one process plays every rank, as
tools/exp_shard_local.py does -- each rank's local step into its slot of the gathered-records
buffer, then each rank's dense-output fill (or, recycled, its clear) and its select.

  (a) f32    f32 shards: local + fill/clear + select                        12m + 4n (fill) bytes
  (b) cast   the workaround: shard.float(), (a), the dense result .to(bf16) (a) + 6m + 6n bytes
  (c) bf16   bf16 shards through grace_shard_select_bf16 / _clear_bf16 / grace_fill_bf16
                                                                            10m + 2n (fill) bytes

Each row runs with a fresh zero-filled output per step and with a recycled output (the previous
step's, cleared through its sel_gi list).  The rows alternate in rounds of --steps steps, steady
state (every row carries its own residuals), timed with device events; each row reports the median,
the fastest and the slowest round in us per rank and step.  The phases' mean times come from
--phase-rounds further rounds with an event pair around every phase (each includes the few us an
event costs; an empty phase shows that cost).  The bytes
are counted from the shapes, not measured.  With --lib PATH (an older build of the library, which
lacks the bf16 entry points) row (c) is skipped and (a), (b) still run.

    python tools/bench_shard_bf16.py [--world W] [--rounds R] [--steps S] [--lib PATH] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grace_amd import _lib, ops  # noqa: E402

BF16 = torch.bfloat16
PHASES = ("cast_up", "local", "fill_or_clear", "select", "cast_down")


class _NoEvent:
    """stands in for an event in the rounds that time whole steps (an event costs device time)"""

    @staticmethod
    def record():
        pass


class Row:
    """One (row, mode): its residuals, payload marks, selection lists and, recycled, its outputs."""

    def __init__(self, kind, recycled, world, sizes, n, cap, dev):
        self.kind, self.recycled = kind, recycled
        self.odt = BF16 if kind == "bf16" else torch.float32
        self.res = [torch.zeros(m, device=dev) for m in sizes]
        self.res2 = [torch.zeros(m, device=dev) for m in sizes]
        self.pay = [torch.full((cap,), -1, dtype=torch.int32, device=dev) for _ in sizes]
        self.sel = [[torch.full((world * cap,), -1, dtype=torch.int32, device=dev) for _ in range(2)]
                    for _ in sizes] if recycled else None
        self.out = [None] * world
        self.steps = 0
        self.rounds = []                      # us per rank and step, one per round
        self.phase = {p: [] for p in PHASES}  # us, per rank and step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--ratio", type=float, default=0.001)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--phase-rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = _lib.use(args.lib) if args.lib else _lib.load()
    have_bf16 = hasattr(lib, "grace_shard_select_bf16")
    dev = torch.device("cuda", 0)
    n, W = args.n, args.world
    k = ops.ratio_k(n, args.ratio)
    cap = k
    sizes = [n // W + (1 if r < n % W else 0) for r in range(W)]
    bases = [sum(sizes[:r]) for r in range(W)]
    stride = ops.shard_record_words(cap)
    tab = torch.tensor(sizes + bases, dtype=torch.int64, device=dev)
    recs = torch.full((W * stride,), -1, dtype=torch.int32, device=dev)
    for r in range(W):
        recs[r * stride] = sizes[r]
        recs[r * stride + 1:r * stride + ops.SHARD_HDR] = 0
    gen = torch.Generator(device=dev)
    g16, g32 = [], []
    for j in range(2):       # two rotated gradients, bf16 values: every row computes the same step
        gen.manual_seed(5 + j)
        g16.append(torch.randn(n, device=dev, generator=gen).to(BF16))
        g32.append(g16[-1].float())
    st = ops.new_status_word()
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731

    def step(row, marks):
        """one step of every rank; marks (a list, or None: no events, the timed rounds) gets each rank's
        events: cast up 0-1, local 1-2, fill or clear 3-4, select 4-5, cast down 5-6"""
        timed = marks is not None
        marks = marks if timed else []
        i = row.steps % 2
        for r in range(W):
            e = [ev() if timed else _NoEvent for _ in range(7)]
            lo, hi = bases[r], bases[r] + sizes[r]
            o = r * stride + ops.SHARD_HDR
            vals, idx = recs[o:o + cap].view(torch.float32), recs[o + cap:o + 2 * cap]
            e[0].record()
            if row.kind == "cast":
                g = g16[i][lo:hi].float()
            else:
                g = (g16 if row.kind == "bf16" else g32)[i][lo:hi]
            e[1].record()
            ops.topk_residual_step_swap(g, row.res[r], row.steps > 0, 1.0, 1.0, min(cap, sizes[r]), row.res2[r],
                                        payload=(None, vals, idx))
            row.res[r], row.res2[r] = row.res2[r], row.res[r]
            e[2].record()
            marks.append(e)
        # (the records of all ranks are complete before any select, as after the all-gather)
        for r in range(W):
            e = marks[len(marks) - W + r]
            e[3].record()
            sel = None
            if row.recycled and row.out[r] is not None:
                prev, sel = row.sel[r]
                out = ops.shard_clear(row.out[r], 0, prev)
                row.sel[r] = [sel, prev]
            else:
                out = torch.empty(n, dtype=row.odt, device=dev)
                if row.odt == BF16:
                    ops.fill_bf16(out, 0)
                else:
                    ops.fill(out, 0.0)
                if row.recycled:
                    sel = row.sel[r][0]      # [0]: the list of the output kept below
            e[4].record()
            ops.shard_select(recs, W, r, cap, tab, k, row.res[r], out, 0, row.pay[r], st, sel)
            e[5].record()
            res = out.to(BF16) if row.kind == "cast" else out
            e[6].record()
            row.out[r] = out if row.recycled else None
            if r == 0:
                row.last = res
            del out, res
        row.steps += 1

    kinds = [kd for kd in ("f32", "cast", "bf16") if kd != "bf16" or have_bf16]
    rows = [Row(kd, rec, W, sizes, n, cap, dev) for rec in (False, True) for kd in kinds]
    for _ in range(args.warmup):
        for row in rows:
            step(row, None)
    for _ in range(args.rounds):
        for row in rows:
            torch.cuda.synchronize()
            e0, e1 = ev(), ev()
            e0.record()
            for _s in range(args.steps):
                step(row, None)
            e1.record()
            e1.synchronize()
            row.rounds.append(e0.elapsed_time(e1) * 1e3 / (args.steps * W))
    # the phases, in rounds of their own: an event between two phases costs a few us of device time,
    # which the step times above do not carry
    for _ in range(args.phase_rounds):
        for row in rows:
            torch.cuda.synchronize()
            marks = []
            for _s in range(args.steps):
                step(row, marks)
            torch.cuda.synchronize()
            for name, a, b in (("cast_up", 0, 1), ("local", 1, 2), ("fill_or_clear", 3, 4), ("select", 4, 5),
                               ("cast_down", 5, 6)):
                row.phase[name].append(statistics.mean(e[a].elapsed_time(e[b]) * 1e3 for e in marks))
    torch.cuda.synchronize()
    # the rows ran the same steps on the same values: (c)'s result is (a)'s rounded once
    by = {(row.kind, row.recycled): row for row in rows}
    checks = {}
    for rec in (False, True):
        a = by[("f32", rec)].last.cpu().to(BF16).view(torch.int16).to(dev)
        checks[f"cast_equals_f32_rounded_{'recycled' if rec else 'fresh'}"] = bool(
            torch.equal(by[("cast", rec)].last.view(torch.int16), a))
        if have_bf16:
            checks[f"bf16_equals_f32_rounded_{'recycled' if rec else 'fresh'}"] = bool(
                torch.equal(by[("bf16", rec)].last.view(torch.int16), a))
    status = ops.status_take(st)
    result = {"n": n, "ratio": args.ratio, "k": k, "world": W, "rounds": args.rounds, "steps_per_round": args.steps,
              "phase_rounds": args.phase_rounds,
              "device": torch.cuda.get_device_name(dev), "library": args.lib or _lib.LIB_PATH,
              "bf16_entry_points": have_bf16, "status_word": status, "checks": checks, "rows": {}}
    print(f"n = {n}, k = {k}, W = {W}: one process plays every rank, no collective; {args.rounds} rounds of "
          f"{args.steps} steps, {result['device']}; library {result['library']}")
    print("us per rank and step (median round, fastest, slowest); phases: mean us per rank and step, event cost "
          "included (median of the phase rounds)")
    print(f"{'row':<6}{'output':<10}{'median':>9}{'min':>9}{'max':>9}  " + "".join(f"{p:>15}" for p in PHASES))
    for row in rows:
        v = row.rounds
        ph = {p: round(statistics.median(row.phase[p]), 1) for p in PHASES}
        mode = "recycled" if row.recycled else "fresh"
        result["rows"][f"{row.kind}_{mode}"] = {"us_median": round(statistics.median(v), 1), "us_min": round(min(v), 1),
                                                "us_max": round(max(v), 1), "phases_us": ph}
        print(f"{row.kind:<6}{mode:<10}{statistics.median(v):>9.1f}{min(v):>9.1f}{max(v):>9.1f}  "
              + "".join(f"{ph[p]:>15.1f}" for p in PHASES))
    if not have_bf16:
        print("bf16   skipped: this library has no bf16 sharded entry points")
    print(f"checks: {checks}; status word {status}")
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    if status or not all(checks.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
