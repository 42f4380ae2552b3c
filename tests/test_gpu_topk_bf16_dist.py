"""bfloat16 gradients through grace_amd.dist's communicator and memories with
grace_amd.topk_bf16.TopKCompressor: Allgather(TopKCompressor, ResidualMemory | NoneMemory).step at
world 1 and world 2, and TopKCompressor.compress / decompress by hand.

The specification: every result is what the f32 path gives for the gradient
widened to f32.  The payload and the residual are f32, bit-equal to the oracle's on the upcast
gradient; the dense result has the gradient's dtype and shape and is the f32 result rounded once by
torch's CPU ``.to(torch.bfloat16)`` -- at world > 1 after the rank-ordered sum and the division."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import grace_oracle as O
from tests.golden_util import same_bits
from tests.test_gpu_topk_bf16 import _inputs, _np, check_dense, check_topk

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
RATIO = 0.01
SHAPES = {32768: (128, 256), (1 << 20) + 7: ((1 << 20) + 7,)}   # one workgroup; sampled, guarded tail


def _comm(memory, world=1, **kw):
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.topk_bf16 import TopKCompressor
    return Allgather(TopKCompressor(RATIO, **kw), memory, world)


def _residual_steps(n, beta, gamma, kind, **kw):
    """Three steps of one name; (results, residual after each step) checked against the oracle."""
    from grace_amd.dist.memory.residual import ResidualMemory
    comm = _comm(ResidualMemory(beta, gamma), **kw)
    k = O.ratio_k(n, RATIO)
    res, outs = None, []
    for s in range(3):
        b, up = _inputs(n, kind, 100 * s + 7)
        g = b.to(DEV).view(SHAPES[n])
        out = comm.step(g, "w")
        t = O.residual_compensate(up, res, beta, gamma).ravel()
        dec = O.sparse_decode(*O.topk_select(t, k), n)
        res = O.residual_update(t, dec)
        r = comm.memory.residuals["w"]
        assert out.dtype == BF16 and out.shape == g.shape and out.data_ptr() != g.data_ptr()
        assert r.dtype == torch.float32 and r.numel() == n
        assert same_bits(_np(r), res), f"residual differs at step {s}"
        check_dense(out.reshape(-1), O.python_sum([dec]))
        outs.append(out)
    return comm, outs


@pytest.mark.parametrize("n", sorted(SHAPES))
@pytest.mark.parametrize("beta,gamma,kind", [(1.0, 1.0, "normal"), (0.9, 0.5, "special")])
@pytest.mark.parametrize("recycle", [True, "always"], ids=["default", "always"])
def test_bf16_residual_step_world1(n, beta, gamma, kind, recycle):
    """recycle_output="always" must not raise on bf16 and changes nothing: a bf16 result is never
    recycled (the three results are distinct buffers, checked while all three are alive)."""
    comm, outs = _residual_steps(n, beta, gamma, kind, recycle_output=recycle)
    assert len({o.data_ptr() for o in outs}) == 3
    assert comm.compressor._recycler.hits == 0 and comm.compressor._recycler.dense_hits == 0


@pytest.mark.parametrize("n", sorted(SHAPES))
@pytest.mark.parametrize("recycle", [True, "always"], ids=["default", "always"])
def test_bf16_nomemory_step_world1(n, recycle):
    from grace_amd.dist.memory.none import NoneMemory
    comm = _comm(NoneMemory(), recycle_output=recycle)
    k = O.ratio_k(n, RATIO)
    for s in range(3):
        b, up = _inputs(n, "special" if s == 1 else "normal", 100 * s + 9)
        g = b.to(DEV).view(SHAPES[n])
        out = comm.step(g, "w")
        assert out.dtype == BF16 and out.shape == g.shape
        check_dense(out.reshape(-1), O.python_sum([O.sparse_decode(*O.topk_select(up, k), n)]))
        del out      # dropped: an f32 step would get this buffer back
    assert comm.compressor._recycler.hits == 0


def test_bf16_step_takes_no_placement_probe(monkeypatch):
    """With the placement threshold lowered below n, an f32 step would call ops.pick_pair on its
    first step; a bf16 step does not (its result is not kept), and place_probes stays empty."""
    from grace_amd import ops

    def boom(*a, **kw):
        raise AssertionError("ops.pick_pair called on a bfloat16 step")
    monkeypatch.setattr(ops, "PLACE_MIN_N", 1 << 16)
    monkeypatch.setattr(ops, "PLACE_PROBE", True)
    monkeypatch.setattr(ops, "pick_pair", boom)
    comm, _ = _residual_steps((1 << 20) + 7, 1.0, 1.0, "normal")
    assert comm.compressor.place_probes == {}


def test_bf16_four_calls_by_hand():
    """compress on a bf16 tensor returns the oracle's f32 payload; decompress decodes to f32."""
    from grace_amd.topk_bf16 import TopKCompressor
    n = 100003
    b, up = _inputs(n, "normal", n + 3)
    c = TopKCompressor(RATIO)
    (vals, idx), ctx = c.compress(b.to(DEV).view(-1, 1), "w")
    k = O.ratio_k(n, RATIO)
    check_topk(up, k, vals, idx)
    dec = c.decompress([vals, idx], ctx)
    assert dec.dtype == torch.float32 and dec.shape == (n, 1)
    assert same_bits(_np(dec).ravel(), O.sparse_decode(*O.topk_select(up, k), n))


def test_gradient_dtype_may_change_between_steps():
    """f32, bf16, f32 steps of one name: the f32 residual carries through both paths."""
    from grace_amd.dist.memory.residual import ResidualMemory
    n = 100003
    comm = _comm(ResidualMemory())
    res = None
    for s, dtype in enumerate((torch.float32, BF16, torch.float32)):
        b, up = _inputs(n, "normal", 900 + s)
        g = b.to(DEV) if dtype == BF16 else torch.from_numpy(up.copy()).to(DEV)
        out = comm.step(g, "w")
        _, _, _, res, exp = O.topk_residual_step(up, res, RATIO)
        assert out.dtype == dtype and comm.memory.residuals["w"].dtype == torch.float32
        assert same_bits(_np(comm.memory.residuals["w"]), res), s
        if dtype == BF16:
            check_dense(out, exp)
        else:
            assert same_bits(_np(out), exp), s


def test_f32_steps_are_the_parent_class_steps():
    """A float32 gradient through the bf16-capable class takes grace_amd.dist's TopKCompressor path:
    the same results and residuals bit for bit, recycling included (NoneMemory, world 1)."""
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.topk import TopKCompressor as F32TopK
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    n = 100003
    for make in (ResidualMemory, NoneMemory):
        a, b = _comm(make()), Allgather(F32TopK(RATIO), make(), 1)
        for s in range(3):
            g = torch.from_numpy(_inputs(n, "normal", 950 + s)[1].copy()).to(DEV)
            oa, ob = a.step(g, "w"), b.step(g, "w")
            assert oa.dtype == torch.float32 and torch.equal(oa.view(torch.int32), ob.view(torch.int32)), s
            if make is ResidualMemory:
                assert torch.equal(a.memory.residuals["w"].view(torch.int32), b.memory.residuals["w"].view(torch.int32))
            del oa, ob
        assert a.compressor._recycler.hits == b.compressor._recycler.hits


def test_float16_is_still_refused():
    from grace_amd.topk_bf16 import TopKCompressor
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    h = torch.ones(4096, dtype=torch.float16, device=DEV)
    for mem in (ResidualMemory(), NoneMemory()):
        with pytest.raises(TypeError):
            _comm(mem).step(h, "w")
    with pytest.raises(TypeError):
        TopKCompressor(RATIO).compress(h, "w")


# ------------------------------------------------------------------------------- world 2
W2_SIZES = (5003, (1 << 20) + 7)
W2_CONFIGS = ("spare", "nospare", "none", "lowered")


def _w2_grad(n, rank, s):
    g = np.random.default_rng(7000 + 10 * rank + s + n % 1000).standard_normal(n).astype(np.float32)
    return torch.from_numpy(g).to(BF16)


def _w2_worker(rank, path, outdir):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=2)
    torch.cuda.set_device(0)
    from grace_amd import ops
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    calls = {"scatter": 0, "narrow": 0, "sorted_bf16": 0}
    scatter, narrow, grouped = ops.sparse_aggregate, ops.f32_to_bf16, ops.sparse_aggregate_sorted

    def count(name, f, when=lambda a, kw: True):
        def g(*a, **kw):
            calls[name] += 1 if when(a, kw) else 0
            return f(*a, **kw)
        return g
    ops.sparse_aggregate, ops.f32_to_bf16 = count("scatter", scatter), count("narrow", narrow)
    ops.sparse_aggregate_sorted = count("sorted_bf16", grouped, lambda a, kw: kw.get("out_dtype") == BF16)
    limit = ops.SORT_PAYLOAD_MAX_N
    res = {}
    for n in W2_SIZES:
        for cfg in W2_CONFIGS:
            ops.SORT_PAYLOAD_MAX_N = (1 << 16) if cfg == "lowered" else limit
            mem = NoneMemory() if cfg == "none" else ResidualMemory(keep_spare=cfg != "nospare")
            comm = _comm(mem, 2)
            before = dict(calls)
            for s in range(2):
                out = comm.step(_w2_grad(n, rank, s).to(DEV), "w")
                assert out.dtype == BF16 and out.shape == (n,)
                res[f"{n}_{cfg}_out{s}"] = out.view(torch.int16).cpu().numpy()
                if cfg != "none":
                    assert mem.residuals["w"].dtype == torch.float32
                    res[f"{n}_{cfg}_res{s}"] = mem.residuals["w"].cpu().numpy()
            res[f"{n}_{cfg}_calls"] = np.array([calls[c] - before[c] for c in ("scatter", "narrow", "sorted_bf16")])
            if cfg in ("spare", "lowered"):   # the first step's residual, retired by the second step
                spare = mem._spare["w"][0]
                res[f"{n}_{cfg}_spare_f32"] = np.array([spare.dtype == torch.float32 and spare.numel() == n])
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


def test_bf16_steps_world2():
    """Two gloo processes on one device, two steps per configuration and size: ResidualMemory with
    and without the spare buffer, NoneMemory (the bf16-only fused branch), and ResidualMemory with
    ops.SORT_PAYLOAD_MAX_N lowered to 2^16 (above it the f32 scatter aggregate, then
    ops.f32_to_bf16).  Expected: each rank's oracle step on its upcast gradient, then
    python_sum(decs) / 2 narrowed once."""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_w2_worker, args=(os.path.join(tmp, "rdv"), tmp), nprocs=2, join=True)
        zs = [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(2)]
    for n in W2_SIZES:
        k = O.ratio_k(n, RATIO)
        big = n > (1 << 16)
        for z in zs:
            for cfg in W2_CONFIGS:
                scatter_path = cfg == "lowered" and big
                assert z[f"{n}_{cfg}_calls"].tolist() == ([2, 2, 0] if scatter_path else [0, 0, 2]), (n, cfg)
            assert z[f"{n}_spare_spare_f32"].all() and z[f"{n}_lowered_spare_f32"].all(), n
        res = [None, None]
        for s in range(2):
            ups = [_w2_grad(n, r, s).float().numpy() for r in range(2)]
            decs, plain = [], []
            for r in range(2):
                t, vals, idx, res[r], _ = O.topk_residual_step(ups[r], res[r], RATIO)
                decs.append(O.sparse_decode(vals, idx, n))
                plain.append(O.sparse_decode(*O.topk_select(ups[r], k), n))
            exp = {True: (O.python_sum(decs) / np.float32(2)).astype(np.float32),
                   False: (O.python_sum(plain) / np.float32(2)).astype(np.float32)}
            for cfg in W2_CONFIGS:
                for r in range(2):
                    out = torch.from_numpy(zs[r][f"{n}_{cfg}_out{s}"]).view(BF16)
                    check_dense(out, exp[cfg != "none"])
                    if cfg != "none":
                        assert same_bits(zs[r][f"{n}_{cfg}_res{s}"], res[r]), (n, cfg, s, r)
                assert np.array_equal(zs[0][f"{n}_{cfg}_out{s}"], zs[1][f"{n}_{cfg}_out{s}"]), (n, cfg, s)
            for r in range(2):
                for cfg in ("nospare", "lowered"):
                    assert np.array_equal(zs[r][f"{n}_{cfg}_out{s}"], zs[r][f"{n}_spare_out{s}"]), (n, cfg, s, r)
                    assert same_bits(zs[r][f"{n}_{cfg}_res{s}"], zs[r][f"{n}_spare_res{s}"]), (n, cfg, s, r)
