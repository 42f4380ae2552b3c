"""DGC on a bfloat16 gradient against today's workaround (cast, f32 path, cast back) and against the
f32 path alone, in one process (no subprocesses), timed with device events.

  step        the world-1 fused step, 1 %, momentum 0.9, steady state (the state carried), at 2^26
              and 2^20 elements          bf16: ops.dgc_step_w1_fused(g)
                                         cast: ops.dgc_step_w1_fused(g.float()) ... out.to(bfloat16)
                                         f32 : ops.dgc_step_w1_fused(g32)
  compensate  r = m r + g, a = a + r in place at 2^26
                                         bf16: ops.dgc_compensate(g, r, a)
                                         cast: ops.dgc_compensate(g.float(), r, a)
                                         f32 : ops.dgc_compensate(g32, r, a)
  decode      W = 8 gathered records of a 1 % selection (grace_dgc_write_capped's), summed and averaged,
              at 2^26 and at 50,000 (launch bound: reported only)
                                         bf16: ops.sparse_aggregate_capped(..., out_dtype=bfloat16)
                                         cast: ops.f32_to_bf16(ops.sparse_aggregate_capped(...))

Bytes are counted from the launches' arguments, not measured; the sample's
gathers and the threshold kernels (under 1 % of the step's bytes) are left out.  Three rotated
gradients per size, as bench.py rotates its buffers; every row is warmed up before it is timed; the
variants of a row group alternate in rounds of --steps calls; each row reports the median, fastest
and slowest round in microseconds per call, the bytes moved and the share of the 8 TB/s peak.

--alt-lib PATH adds a fourth variant to the step and decode rows: the bf16 call on another build of
the library (grace_amd._lib.use), for A/B of a kernel variant inside the same alternation; its first
result is compared with this build's.

    python tools/bench_dgc_bf16.py [--sizes 67108864,1048576] [--rounds R] [--steps S] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grace_amd import _lib, ops  # noqa: E402

W = 8
RATIO, MOM = 0.01, 0.9
PEAK = 8e12
BF16 = torch.bfloat16
F32 = torch.float32
NAMES = ("bf16", "cast", "f32")
ALT = "bf16 alt"


def records(g32, n, dev):
    """W records of a 1 % DGC selection (the three gradients in turn, scaled apart), gathered
    rank-major at the capacity of the largest count; (recs, cap, entries in all)."""
    ts = [g32[w % 3] * (1.0 + 0.25 * w) for w in range(W)]
    wss, counts = [], []
    for w, t in enumerate(ts):
        ws = ops.dgc_threshold_dev(t, RATIO, seed=100 + w)
        counts.append(int(ws[8:12].view(torch.int32).item()))
        wss.append(ws.clone())
    cap = max(max(counts), 1)
    recs = torch.cat([ops.dgc_write_capped(t, ws, cap) for t, ws in zip(ts, wss)])
    return recs, cap, sum(counts)


class Step:
    """One variant of the steady-state step: its own carried state."""

    def __init__(self, grads, mode):
        self.g, self.mode, self.r, self.a = grads, mode, None, None

    def __call__(self, i):
        g = self.g[i % 3]
        if self.mode == "cast":
            g = g.float()
        out, self.r, self.a = ops.dgc_step_w1_fused(g, self.r, self.a, self.r is not None, MOM, RATIO, seed=i)
        return out.to(BF16) if self.mode == "cast" else out


def time_rows(fns, args, alt=None):
    """fns: the row group's variants; alt: a last variant to run on the --alt-lib build."""
    libs = [_lib.LIB_PATH] * len(fns)
    if alt is not None and args.alt_lib:
        fns, libs = list(fns) + [alt], libs + [args.alt_lib]
    for i in range(args.warmup):
        for f, lib in zip(fns, libs):
            _lib.use(lib)
            f(i)
    us = [[] for _ in fns]
    for _ in range(args.rounds):
        for v, f in enumerate(fns):      # the variants of one row group alternate
            torch.cuda.synchronize()
            _lib.use(libs[v])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                f(i)
            e1.record()
            e1.synchronize()
            us[v].append(e0.elapsed_time(e1) / args.steps * 1e3)
    _lib.use(_lib.LIB_PATH)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"{1 << 26},{1 << 20}")
    ap.add_argument("--decode-sizes", default=f"{1 << 26},50000")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--alt-lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(dev)}: {args.rounds} rounds of {args.steps} calls per row, us per call "
             f"(median, min, max of the rounds); bytes counted, share of {PEAK / 1e12:.0f} TB/s; decode rows: W = {W}",
             f"{'n':>10} {'row':<18}{'median us':>11}{'min':>10}{'max':>10}{'MB moved':>10}{'of peak':>9}"]
    verdicts = []

    def report(n, row, us, moved):
        med = [statistics.median(u) for u in us]
        names = NAMES[:len(moved)] + (ALT,)
        moved = tuple(moved) + (moved[0],)
        for v, u in enumerate(us):
            lines.append(f"{n:>10} {row + ' ' + names[v]:<18}{med[v]:>11.1f}{min(u):>10.1f}{max(u):>10.1f}"
                         f"{moved[v] / 1e6:>10.1f}{moved[v] / (med[v] * 1e-6) / PEAK:>9.1%}")
        verdicts.append(f"{n}: {row}: bf16 median {med[0]:.1f} us against the cast row's fastest round "
                        f"{min(us[1]):.1f} us ({'below' if med[0] < min(us[1]) else 'NOT below'}); cast / bf16 = "
                        f"{med[1] / med[0]:.2f}x" + (f", f32 / bf16 = {med[2] / med[0]:.2f}x" if len(moved) == 4 else ""))

    sizes = [int(s) for s in args.sizes.split(",") if s]
    dsizes = [int(s) for s in args.decode_sizes.split(",") if s]
    for n in sorted(set(sizes) | set(dsizes), reverse=True):
        gen = torch.Generator(device=dev)
        g16, g32 = [], []
        for j in range(3):
            gen.manual_seed(j + 1)
            g16.append((torch.randn(n, device=dev, generator=gen) * 0.01).to(BF16))
            g32.append(g16[-1].float())
        if n in sizes:
            if args.alt_lib:   # one step from the same state on both builds: the same bits
                a = ops.dgc_step_w1_fused(g16[0], g32[1], g32[2], True, MOM, RATIO, seed=1)
                _lib.use(args.alt_lib)
                b = ops.dgc_step_w1_fused(g16[0], g32[1], g32[2], True, MOM, RATIO, seed=1)
                _lib.use(_lib.LIB_PATH)
                assert all(torch.equal(x.view(torch.int16 if x.dtype == BF16 else torch.int32),
                                       y.view(torch.int16 if y.dtype == BF16 else torch.int32)) for x, y in zip(a, b))
                del a, b
            us = time_rows([Step(g16, "bf16"), Step(g16, "cast"), Step(g32, "f32")], args, alt=Step(g16, "bf16"))
            report(n, "step", us, (20 * n, 36 * n, 24 * n))
        if n == max(sizes):
            state = [(torch.zeros(n, device=dev), torch.zeros(n, device=dev)) for _ in range(3)]
            fns = [lambda i: ops.dgc_compensate(g16[i % 3], *state[0], True, MOM),
                   lambda i: ops.dgc_compensate(g16[i % 3].float(), *state[1], True, MOM),
                   lambda i: ops.dgc_compensate(g32[i % 3], *state[2], True, MOM)]
            report(n, "compensate", time_rows(fns, args), (18 * n, 26 * n, 20 * n))
            del state, fns
        if n in dsizes:
            recs, cap, total = records(g32, n, dev)
            stat = torch.empty(2, dtype=torch.int32, device=dev)
            fns = [lambda i: ops.sparse_aggregate_capped(recs, cap, W, n, W, stat, out_dtype=BF16),
                   lambda i: ops.f32_to_bf16(ops.sparse_aggregate_capped(recs, cap, W, n, W, stat))]
            # bf16: indices once for the boundaries, entries once, 2 n out.  cast: 4 n fill, per entry 8 read +
            # 8 out read-modify-write + 4 tag, the divide's 4 idx + 4 tag + 8, then 4 n + 2 n to narrow
            moved = (2 * n + 12 * total, 10 * n + 36 * total)
            if args.alt_lib:
                a = fns[0](0)
                _lib.use(args.alt_lib)
                b = fns[0](0)
                _lib.use(_lib.LIB_PATH)
                assert torch.equal(a.view(torch.int16), b.view(torch.int16))
                del a, b
            report(n, f"decode ({total} entries)", time_rows(fns, args, alt=fns[0]), moved)
            del recs, fns
        del g16, g32
        torch.cuda.empty_cache()
    text = "\n".join(lines + verdicts) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
