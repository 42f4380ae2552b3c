"""The error-bounded variable-width codec (grace_amd/csrc/inceptionn.hip) at 2^26
elements, f32 and bf16, b = 10, in one process, timed with device events, on three gradients: normal of
scale 1e-3, normal of scale 1e-1, and the worst case in which every element is sent whole (tag 3):

  compress   ops.inceptionn_compress                  the capacity-sized buffer; no host read
  step       ops.inceptionn_step_w1                   the world-1 step, dense result in g's dtype
  decode     ops.inceptionn_decode_aggregate, W = 8   eight payloads, averaged, result in g's dtype

Beside each row: (a) the row's bytes over 8 TB/s, counted from the launches' arguments and the payload's
word 0, not measured (compress reads x and writes the payload; the step reads x and writes the result; the
decode reads W payloads and writes the result), and the rate those bytes imply; (b) the nearest streaming
codec of this library on the same n (natural_compress, cast_step_w1 in natural mode, natural_decompress
at W = 8; they move 4n or 2n + n, 8n or 4n, and 8n + 4n or 2n bytes); (c) the eager-PyTorch composition a
user has without the codec (masks, nonzero gathers, shifts; for the decode masked scatters a rank).  The
variants of a row alternate in rounds of --steps calls (a tenth of them for the eager composition); each
reports the median, fastest and slowest round in microseconds per call.

    python tools/bench_inceptionn.py [--n N] [--rounds R] [--steps S] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grace_amd import ops  # noqa: E402

W, B = 8, 10
PEAK = 8e12
LO, MID = 127 - B, 127 - B + (B + 1) // 2


def eager_parts(g):
    x = g.float().view(-1)
    u = x.view(torch.int32)
    e = (u >> 23) & 255
    return x, (u >> 31) & 1, (e >= LO).to(torch.uint8) + (e >= MID) + (e >= 127)


def eager_compress(g):
    """(tags four to a byte, tag-3 values, tag-2 codes, tag-1 codes); n is a multiple of 4"""
    x, s, tag = eager_parts(g)
    t4 = tag.view(-1, 4)
    a2, a1 = x[tag == 2].abs(), x[tag == 1].abs()
    c2 = (a2 * 2.0 ** 15).floor().to(torch.int32) | (s[tag == 2] << 15)
    c1 = (a1 * 2.0 ** (134 - MID)).floor().to(torch.int32) | (s[tag == 1] << 7)
    return t4[:, 0] | t4[:, 1] << 2 | t4[:, 2] << 4 | t4[:, 3] << 6, x[tag == 3], c2.to(torch.int16), c1.to(torch.uint8)


def eager_step(g):
    x, _, tag = eager_parts(g)
    q2, q1 = (x * 2.0 ** 15).trunc() * 2.0 ** -15, (x * 2.0 ** (134 - MID)).trunc() * 2.0 ** (MID - 134)
    return torch.where(tag == 3, x, torch.where(tag == 2, q2, torch.where(tag == 1, q1, torch.zeros_like(x)))).to(g.dtype)


def eager_decode(parts, n, dtype):
    acc = torch.zeros(n, device=parts[0][0].device)
    for tags, v3, c2, c1 in parts:
        tag = torch.stack([tags & 3, (tags >> 2) & 3, (tags >> 4) & 3, tags >> 6], 1).view(-1)
        d = torch.zeros_like(acc)
        d[tag == 3] = v3
        c2, c1 = c2.to(torch.int32) & 0xFFFF, c1.to(torch.int32)
        d[tag == 2] = (c2 & 0x7FFF).float() * 2.0 ** -15 * (1 - 2 * (c2 >> 15)).float()
        d[tag == 1] = (c1 & 0x7F).float() * 2.0 ** (MID - 134) * (1 - 2 * (c1 >> 7)).float()
        acc = acc + d
    return (acc / W).to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n // 4 * 4
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    emit(f"{torch.cuda.get_device_name(dev)}: n = {n}, b = {B}, {args.rounds} rounds of {args.steps} calls per row, us per "
         f"call (median, min, max of the rounds); bytes counted; (a) = bytes / {PEAK / 1e12:.0f} TB/s; decode: W = {W}")
    emit(f"{'row':<44}{'B/elem':>7}{'(a) us':>9}{'median us':>13}{'min':>13}{'max':>13}{'TB/s':>7}{'of peak':>9}")
    ratios = []
    gen = torch.Generator(device=dev).manual_seed(1)
    base = [torch.randn(n, device=dev, generator=gen) for _ in range(3)]
    for dtype, name, sz in ((torch.float32, "f32", 4), (torch.bfloat16, "bf16", 2)):
        for kind, scale in (("1e-3", 1e-3), ("1e-1", 1e-1), ("tag3", None)):
            g = [(t * scale if scale else t.abs() + 1).to(dtype) for t in base]
            pays = [ops.inceptionn_compress(g[w % 3], B) for w in range(W)]
            total = ops.inceptionn_payload_bytes(pays[0])
            stride = max(ops.inceptionn_payload_bytes(p) for p in pays)
            wire = torch.zeros(W * stride, dtype=torch.uint8, device=dev)
            for w, p in enumerate(pays):
                wire.view(W, stride)[w, :ops.inceptionn_payload_bytes(p)] = p[:ops.inceptionn_payload_bytes(p)]
            read = sum(ops.inceptionn_payload_bytes(p) for p in pays)
            del pays
            parts = [eager_compress(g[w % 3]) for w in range(W)]
            ncodes = torch.cat([ops.natural_compress(g[w % 3]) for w in range(W)])
            rows = {
                "compress": ((sz * n + total) / n, sz + 1, [
                    lambda i: ops.inceptionn_compress(g[i % 3], B), lambda i: ops.natural_compress(g[i % 3]),
                    lambda i: eager_compress(g[i % 3])]),
                "step": (2 * sz, 2 * sz, [
                    lambda i: ops.inceptionn_step_w1(g[i % 3], B), lambda i: ops.cast_step_w1(g[i % 3], 0, i),
                    lambda i: eager_step(g[i % 3])]),
                "decode": ((read + sz * n) / n, W + sz, [
                    lambda i: ops.inceptionn_decode_aggregate(wire, W, n, B, divisor=float(W), out_dtype=dtype),
                    lambda i: ops.natural_decompress(ncodes, n, 0, world=W, aggregate=True, divisor=float(W),
                                                     out_dtype=dtype),
                    lambda i: eager_decode(parts, n, dtype)]),
            }
            emit(f"{name} {kind}: the payload is {total} bytes, {total / (4 * n):.1%} of the float32 bytes")
            for row, (bpe, nat_bpe, fns) in rows.items():
                steps = [args.steps, args.steps, max(1, args.steps // 10)]
                us = [[] for _ in fns]
                for f in fns:
                    for i in range(args.warmup):
                        f(i)
                for _ in range(args.rounds):
                    for v, f in enumerate(fns):      # the variants of one row alternate
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(steps[v]):
                            f(i)
                        e1.record()
                        e1.synchronize()
                        us[v].append(e0.elapsed_time(e1) / steps[v] * 1e3)
                med = [statistics.median(u) for u in us]
                tag = f"{name} {kind} {row}"
                for v, what in enumerate(("inceptionn", "(b) natural", "(c) eager")):
                    b = (bpe, nat_bpe, None)[v]
                    floor = f"{b * n / PEAK * 1e6:>9.1f}" if b else f"{'':>9}"
                    rate = f"{b * n / (med[v] * 1e-6) / 1e12:>7.2f}{b * n / (med[v] * 1e-6) / PEAK:>9.1%}" if b else ""
                    emit(f"{tag + ' ' + what:<44}{(f'{b:.2f}' if b else ''):>7}{floor}{med[v]:>13.1f}"
                         f"{min(us[v]):>13.1f}{max(us[v]):>13.1f}{rate}")
                ratios.append(f"{tag}: rate / natural's rate = {(bpe / med[0]) / (nat_bpe / med[1]):.2f}, time / natural's = "
                              f"{med[0] / med[1]:.2f}x, eager / inceptionn = {med[2] / med[0]:.1f}x")
            del wire, parts, ncodes, g
            torch.cuda.empty_cache()
    print("\n".join(ratios), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines + ratios) + "\n")


if __name__ == "__main__":
    main()
