"""Allgather(grace_amd.cast_bf16.X, NoneMemory(), W).step on bfloat16 gradients.

Every result is compared with an f32 grace_amd.dist twin of the same class, stepped on ``g.float()``
under the same name (so both draw the same randoms), rounded once by torch's CPU cast: equal 16-bit
patterns, dtype and shape.  World 1 in this process; world 2 as two gloo processes on one device,
the way tests/test_gpu_quant_bf16_dist.py spawns its ranks, with a mixed pair -- rank 0 steps the
bf16 class on g, rank 1 the f32 class on g.float() -- to show that the two share a wire."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_gpu_topk_bf16 import _bits16

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32
# (class, constructor arguments): every class and every generator it has
CONFIGS = {
    "natural": ("NaturalCompressor", dict()),
    "natural_cpu": ("NaturalCompressor", dict(rng="torch_cpu")),
    "cnat": ("NaturalCompressor_CUDA", dict()),
    "cnat_cpu": ("NaturalCompressor_CUDA", dict(rng="torch_cpu")),
    "cnat_det": ("NaturalCompressor_CUDA", dict(rng="deterministic")),
    "fp16": ("FP16Compressor", dict()),
    "onebit": ("OneBitCompressor", dict()),
    "onebit_quirk": ("OneBitCompressor", dict(compat_uint8_not=True)),
}


def _pair(config, world, average=True):
    """(the cast_bf16 communicator, its f32 grace_amd.dist twin)"""
    from grace_amd import cast_bf16
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor import fp16, natural, onebit
    from grace_amd.dist.memory.none import NoneMemory
    cls, kw = CONFIGS[config]
    new = getattr(cast_bf16, cls)(**kw)
    old = getattr({"N": natural, "F": fp16, "O": onebit}[cls[0]], cls)(**kw)
    assert type(old) is not type(new) and isinstance(new, type(old))
    new.average = old.average = average
    return Allgather(new, NoneMemory(), world), Allgather(old, NoneMemory(), world)


def _grad(shape, seed):
    g = torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * 0.01)
    return g.to(BF16)


def _step_both(new, old, g, name, s):
    """one step of both twins on g / g.float(); the CPU generator (rng="torch_cpu") is reset for each"""
    torch.manual_seed(1234 + s)
    out = new.step(g, name)
    torch.manual_seed(1234 + s)
    ref = old.step(g.float(), name)
    assert ref.dtype == F32
    return out, ref


def _check(out, ref, g):
    assert out.dtype == BF16 and out.shape == g.shape
    assert out.untyped_storage().data_ptr() != g.untyped_storage().data_ptr()
    assert np.array_equal(_bits16(out), _bits16(ref.cpu().to(BF16)))


@pytest.mark.parametrize("shape", [(128, 256), (100003,)], ids=["128x256", "100003"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_world1_steps_equal_the_f32_twin_rounded_once(config, shape):
    new, old = _pair(config, 1)
    outs = []
    for s in range(3):
        g = _grad(shape, 10 * s + len(shape)).to(DEV)
        out, ref = _step_both(new, old, g, "w", s)
        _check(out, ref, g)
        outs.append(out)
    if hasattr(old.compressor, "_step"):
        assert new.compressor._step == old.compressor._step == 3
    assert len({o.data_ptr() for o in outs}) == 3    # held results are distinct tensors


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_world1_non_contiguous_and_odd_views(config):
    """A transposed view and views that start on an odd element (2-byte aligned): made contiguous and
    aligned first; the result has the view's shape."""
    new, old = _pair(config, 1)
    base = _grad((300, 130), 5).to(DEV)
    for s, g in enumerate((base.t(), base[:, 1:], base.view(-1)[1:4100])):
        assert not g.is_contiguous() or g.data_ptr() % 16
        out, ref = _step_both(new, old, g, "v", s)
        _check(out, ref, g)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_special_values_world1(config):
    """+inf, NaN, -0.0 and a run of zeros: NaN results are 0x7FC0 and sit where the twin's are."""
    new, old = _pair(config, 1)
    g = _grad((4099,), 3)
    g[5], g[300], g[1000:1128], g[2000::7] = float("inf"), float("nan"), 0.0, -0.0
    g = g.to(DEV)
    out, ref = _step_both(new, old, g, "w", 0)
    assert out.dtype == BF16 and out.shape == g.shape
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(out.float()), nan) and bool((out.view(torch.int16)[nan] == 0x7FC0).all())
    ok = (~nan).cpu().numpy()
    assert np.array_equal(_bits16(out)[ok], _bits16(ref.cpu().to(BF16))[ok])


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_f32_gradients_take_the_parent_path(config):
    """An f32 gradient through the subclass: the parent's result bit for bit, in f32."""
    new, old = _pair(config, 1)
    for s, shape in enumerate([(128, 256), (4099,)]):
        g = _grad(shape, 40 + s).float().to(DEV)
        torch.manual_seed(7)
        out = new.step(g, "w")
        torch.manual_seed(7)
        ref = old.step(g, "w")
        assert out.dtype == F32 and out.shape == g.shape
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_refusals():
    """float16 raises TypeError in every class; compress by hand and ResidualMemory refuse bf16, and so
    do grace_amd.dist's own classes on the Allgather step."""
    from grace_amd import cast_bf16 as C
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor import fp16, natural, onebit
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    h = torch.ones(4096, dtype=torch.float16, device=DEV)
    b = torch.ones(4096, dtype=BF16, device=DEV)
    for comp in (C.NaturalCompressor(), C.NaturalCompressor_CUDA(), C.FP16Compressor(), C.OneBitCompressor()):
        with pytest.raises(TypeError):
            Allgather(comp, NoneMemory(), 1).step(h, "w")
        with pytest.raises(TypeError):
            comp.compress(b, "w")
        with pytest.raises(TypeError):
            Allgather(comp, ResidualMemory(), 1).step(b, "w")
    for comp in (natural.NaturalCompressor(), natural.NaturalCompressor_CUDA(), fp16.FP16Compressor(),
                 onebit.OneBitCompressor()):
        with pytest.raises(TypeError):
            Allgather(comp, NoneMemory(), 1).step(b, "w")


# ------------------------------------------------------------------------------- world 2
W2_SHAPES = ((128, 256), (100003,))
W2_CASES = [(c, True) for c in ("natural", "natural_cpu", "cnat", "cnat_det", "fp16", "onebit", "onebit_quirk")] + \
    [("natural", False), ("fp16", False), ("onebit", False)]
W2_MIXED = ("natural", "cnat", "fp16", "onebit")


def _w2_grad(shape, rank, s):
    return _grad(shape, 9000 + 10 * rank + s + len(shape))


def _w2_worker(rank, path, outdir):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=2)
    torch.cuda.set_device(0)
    res = {}
    for si, shape in enumerate(W2_SHAPES):
        for config, average in W2_CASES:
            new, old = _pair(config, 2, average)
            for s in range(2):
                g = _w2_grad(shape, rank, s).to(DEV)
                if s == 1 and len(shape) == 2:
                    g = g.t()    # a non-contiguous view on the second step
                out, ref = _step_both(new, old, g, "w", s)
                assert out.dtype == BF16 and out.shape == g.shape and ref.dtype == F32
                key = f"{si}_{config}_{int(average)}_{s}"
                res[key + "_out"] = _bits16(out)
                res[key + "_ref"] = _bits16(ref.cpu().to(BF16))
                res[key + "_sum"] = ref.float().abs().sum().cpu().numpy()
    # the shared wire: rank 0 is a bf16 rank, rank 1 an f32 rank of the same class, in one collective;
    # then both ranks step the f32 class as the reference
    for config in W2_MIXED:
        new, old = _pair(config, 2)
        ref_comm = _pair(config, 2)[1]
        g = _w2_grad(W2_SHAPES[1], rank, 0).to(DEV)
        torch.manual_seed(99)
        out = new.step(g, "m") if rank == 0 else old.step(g.float(), "m")
        torch.manual_seed(99)
        ref = ref_comm.step(g.float(), "m")
        assert out.dtype == (BF16 if rank == 0 else F32)
        res[f"mixed_{config}_out"] = _bits16(out if rank == 0 else out.cpu().to(BF16))
        res[f"mixed_{config}_ref"] = _bits16(ref.cpu().to(BF16))
        if rank == 1:
            assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


def test_world2_steps_equal_the_f32_twin_rounded_once():
    """Two gloo processes on one device, two steps per class, shape and `average`: each rank's bf16
    result is its f32 twin's rounded once (after the rank-ordered sum and the division), both ranks
    hold the same bytes, and without averaging the result is twice the average's size.  In the mixed
    pairs the bf16 rank and the f32 rank exchange one payload format and agree with the all-f32 run."""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_w2_worker, args=(os.path.join(tmp, "rdv"), tmp), nprocs=2, join=True)
        zs = [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(2)]
    for si in range(len(W2_SHAPES)):
        for config, average in W2_CASES:
            for s in range(2):
                key = f"{si}_{config}_{int(average)}_{s}"
                for r in range(2):
                    assert np.array_equal(zs[r][key + "_out"], zs[r][key + "_ref"]), (key, r)
                assert np.array_equal(zs[0][key + "_out"], zs[1][key + "_out"]), key
        for config in ("natural", "fp16", "onebit"):
            for s in range(2):
                avg, tot = zs[0][f"{si}_{config}_1_{s}_sum"], zs[0][f"{si}_{config}_0_{s}_sum"]
                assert 1.9 * avg < tot < 2.1 * avg, (config, s, avg, tot)
    for config in W2_MIXED:
        for r in range(2):
            assert np.array_equal(zs[r][f"mixed_{config}_out"], zs[r][f"mixed_{config}_ref"]), (config, r)
        assert np.array_equal(zs[0][f"mixed_{config}_out"], zs[1][f"mixed_{config}_out"]), config
