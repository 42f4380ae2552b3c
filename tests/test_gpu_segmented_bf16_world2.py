"""grace_amd.segmented_bf16.SegmentedTopK(world_size=2) on bfloat16 gradients, two ranks sharing
cuda:0 over gloo (spawned as tests/test_gpu_w8.py::test_segmented_topk_world spawns its ranks): the
segment list and the planted contents of tests/test_gpu_segmented_bf16.py, two steps and one
in-place step.

Expected, per DESIGN.md §9: every rank's f32 residual is the per-tensor oracle's on that rank's
upcast gradient, bit for bit; the dense result is ((0 + d0) + d1) / 2 in f32 -- Python's rank-ordered
sum of the decoded payloads, then the division -- rounded once to bf16 as torch's CPU cast rounds
(check_dense)."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import grace_oracle as O
from tests.golden_util import same_bits
from tests.test_gpu_segmented_bf16 import EDGE_SIZES, RATIO, edge_grads
from tests.test_gpu_topk_bf16 import check_dense

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
F32 = np.float32
STEPS = 2


def _flat(rank, step):
    return torch.from_numpy(np.concatenate(edge_grads(700 + rank, step))).to(BF16)


def _worker(rank, world, path, outdir):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from grace_amd.segmented_bf16 import SegmentedTopK
    eng = SegmentedTopK(RATIO, world_size=world)
    res = {}
    for s in range(STEPS):
        out = eng.step(_flat(rank, s).cuda(), EDGE_SIZES, "model")
        assert out.dtype == BF16
        res[f"out{s}"] = out.view(torch.int16).cpu().numpy()
        res[f"res{s}"] = eng.residuals["model"].cpu().numpy()
    # in place, as harness.step_segmented runs it (out is the gradient buffer itself)
    eng2 = SegmentedTopK(RATIO, world_size=world)
    g = _flat(rank, 0).cuda()
    assert eng2.step(g, EDGE_SIZES, "model", out=g) is g
    res["inplace0"] = g.view(torch.int16).cpu().numpy()
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_segmented_bf16_world2():
    world = 2
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "rdv"), tmp), nprocs=world, join=True)
        got = [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(world)]
    offs = np.cumsum((0,) + EDGE_SIZES)
    res = [[None] * len(EDGE_SIZES) for _ in range(world)]
    as_bf16 = lambda a: torch.from_numpy(a).view(BF16)   # noqa: E731
    for s in range(STEPS):
        acc = None
        for r in range(world):
            gs = edge_grads(700 + r, s)
            dec = np.empty(offs[-1], F32)
            rr = np.empty(offs[-1], F32)
            for i, g in enumerate(gs):
                a, b = offs[i], offs[i + 1]
                _, vals, idx, res[r][i], _ = O.topk_residual_step(g, res[r][i], RATIO)
                dec[a:b] = O.sparse_decode(vals, idx, b - a)
                rr[a:b] = res[r][i]
            assert same_bits(got[r][f"res{s}"], rr), ("residual", s, r)
            acc = (F32(0) + dec) if acc is None else (acc + dec)
        exp = (acc / F32(world)).astype(F32)
        for r in range(world):
            check_dense(as_bf16(got[r][f"out{s}"]), exp)
        if s == 0:
            for r in range(world):
                check_dense(as_bf16(got[r]["inplace0"]), exp)
