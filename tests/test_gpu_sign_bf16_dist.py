"""bfloat16 gradients through grace_amd.dist's Allgather with grace_amd.sign_bf16's SignSGDCompressor,
SignumCompressor and EFSignSGDCompressor, at world 1 and world 2.

The specification: codes, momentum, residual and mean are the f32 path's on
the gradient widened to f32; the dense result has the gradient's dtype and shape.  The EF-signSGD
mean is the device's own (2 ulp of the exact one: tests/test_gpu_efsign_fused.py), so the residual
and the result are checked exactly given the means the device used, which the tests record by
wrapping ops.efsign_step."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import grace_oracle as O
from tests import sign_bf16_util as U
from tests.test_gpu_efsign_fused import _ulps
from tests.test_gpu_sign_bf16 import _bits, _pm1_bits
from tests.test_gpu_topk_bf16 import _inputs, _np, check_dense

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32
SHAPES = {32768: (128, 256), 100003: (100003,)}
LR_MEM, LR_AGG = 0.1, 0.25


def _comm(kind, world=1):
    from grace_amd import sign_bf16 as S
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.efsignsgd import EFSignSGDMemory
    from grace_amd.dist.memory.none import NoneMemory
    if kind == "ef":
        return Allgather(S.EFSignSGDCompressor(LR_AGG), EFSignSGDMemory(LR_MEM), world)
    if kind == "signum":
        return Allgather(S.SignumCompressor(0.9), NoneMemory(), world)
    return Allgather(S.SignSGDCompressor(wire=kind), NoneMemory(), world)


def _record_means(monkeypatch):
    from grace_amd import ops
    means, real = [], ops.efsign_step

    def wrapped(*a, **kw):
        r = real(*a, **kw)
        means.append(r[0])
        return r
    monkeypatch.setattr(ops, "efsign_step", wrapped)
    return means


@pytest.mark.parametrize("n", sorted(SHAPES))
@pytest.mark.parametrize("wire", ["u8", "bits"])
def test_signsgd_world1(n, wire):
    comm = _comm(wire)
    for s in range(2):
        b, up = _inputs(n, "special" if s else "normal", 40 + s)
        g = b.to(DEV).view(SHAPES[n])
        out = comm.step(g, "w")
        assert out.dtype == BF16 and out.shape == g.shape and out.data_ptr() != g.data_ptr()
        assert np.array_equal(_bits(out), _pm1_bits(O.sign_encode(up)))
        del out
    # a strided view of a (256, 128) tensor: not contiguous
    g = _inputs(32768, "normal", 40)[0].to(DEV).view(256, 128).t()
    out = comm.step(g, "w")
    assert out.dtype == BF16 and out.shape == (128, 256)
    assert np.array_equal(_bits(out), _pm1_bits(O.sign_encode(g.float().cpu().numpy())))
    # compress by hand takes bf16; decompress decodes to f32 as the parent's
    (payload,), ctx = comm.compressor.compress(g.contiguous(), "w")
    dec = comm.compressor.decompress([payload], ctx)
    assert dec.dtype == F32 and dec.shape == (128, 256)
    assert np.array_equal(_np(dec).ravel(), O.sign_decode(O.sign_encode(g.float().cpu().numpy())))


def test_holding_the_signsgd_result_yields_a_distinct_buffer():
    from grace_amd import ops
    comm = _comm("u8")
    g1 = _inputs(32768, "normal", 50)[0].to(DEV)
    g2 = _inputs(32768, "normal", 51)[0].to(DEV)
    held = comm.step(g1, "w")
    kept = _bits(held).copy()
    out2 = comm.step(g2, "w")
    assert out2.data_ptr() != held.data_ptr() and np.array_equal(_bits(held), kept)
    view = out2[1:]                      # a view keeps the storage alive as well
    del out2
    out3 = comm.step(g1, "w")
    assert out3.data_ptr() != view.data_ptr() - 2 and np.array_equal(_bits(out3), kept)
    del held, view, out3                 # dropped: the next two steps may share one buffer
    p = comm.step(g1, "w").data_ptr()
    assert comm.step(g2, "w").data_ptr() == p or not ops.REUSE_OK


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_signum_world1(n):
    comm = _comm("signum")
    prev = None
    for s in range(3):
        b, up = _inputs(n, "normal", 60 + s)
        g = b.to(DEV).view(SHAPES[n])
        out = comm.step(g, "w")
        prev = O.signum_momentum(up, prev, 0.9)
        m = comm.compressor.momentums["w"]
        assert out.dtype == BF16 and out.shape == g.shape
        assert m.dtype == F32 and m.numel() == n and np.array_equal(_np(m).view(np.uint32), prev.view(np.uint32))
        assert np.array_equal(_bits(out), _pm1_bits(O.sign_encode(prev)))


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_efsignsgd_world1(n, monkeypatch):
    means = _record_means(monkeypatch)
    comm = _comm("ef")
    res = None
    for s in range(3):
        b, up = _inputs(n, "normal", 70 + s)
        g = b.to(DEV).view(SHAPES[n])
        out = comm.step(g, "w")
        m = _np(means[-1])
        t, _, _, res, dense = U.ef_step(up, res, LR_MEM, m, LR_AGG)
        assert _ulps(m[0], U.exact_mean(t)) <= 2, s
        r = comm.memory.residuals["w"]
        assert out.dtype == BF16 and out.shape == g.shape and out.data_ptr() != g.data_ptr()
        assert r.dtype == F32 and r.numel() == n and U.same_bits_nan(_np(r), res), s
        check_dense(out.reshape(-1), dense)
    assert len(means) == 3               # one fused step each


@pytest.mark.parametrize("kind", ["ef", "signum"])
def test_gradient_dtype_may_change_between_steps(kind, monkeypatch):
    """f32, bf16, f32 steps of one name share the f32 state: the f32 steps are the parent's unfused
    path (EF-signSGD: its own abs_mean, read back from a compress by hand on the same t)."""
    from grace_amd import ops
    means = _record_means(monkeypatch)
    n = 100003
    comm = _comm(kind)
    state = None
    for s, dtype in enumerate((F32, BF16, F32)):
        b, up = _inputs(n, "normal", 80 + s)
        g = b.to(DEV) if dtype == BF16 else torch.from_numpy(up.copy()).to(DEV)
        out = comm.step(g, "w")
        assert out.dtype == dtype and out.shape == (n,)
        if kind == "signum":
            state = O.signum_momentum(up, state, 0.9)
            assert comm.compressor.momentums["w"].dtype == F32
            assert np.array_equal(_np(comm.compressor.momentums["w"]).view(np.uint32), state.view(np.uint32)), s
            assert np.array_equal(_np(out.float()), O.sign_aggregate([O.sign_decode(O.sign_encode(state))])), s
            continue
        t = O.efsign_compensate(up, state, LR_MEM)
        m = _np(means[-1]) if dtype == BF16 else _np(ops.abs_mean(torch.from_numpy(t).to(DEV)))
        _, _, _, state, dense = U.ef_step(up, state, LR_MEM, m, LR_AGG)
        r = comm.memory.residuals["w"]
        assert r.dtype == F32 and U.same_bits_nan(_np(r), state), s
        if dtype == BF16:
            check_dense(out, dense)
        else:
            assert U.same_bits_nan(_np(out), dense), s
    assert kind == "signum" or len(means) == 1        # only the bf16 step is fused


def test_f32_gradients_give_the_parent_classes_results():
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.efsignsgd import EFSignSGDCompressor
    from grace_amd.dist.compressor.signsgd import SignSGDCompressor
    from grace_amd.dist.compressor.signum import SignumCompressor
    from grace_amd.dist.memory.efsignsgd import EFSignSGDMemory
    from grace_amd.dist.memory.none import NoneMemory
    n = 100003
    pairs = [(_comm("u8"), Allgather(SignSGDCompressor(), NoneMemory(), 1)),
             (_comm("bits"), Allgather(SignSGDCompressor(wire="bits"), NoneMemory(), 1)),
             (_comm("signum"), Allgather(SignumCompressor(0.9), NoneMemory(), 1)),
             (_comm("ef"), Allgather(EFSignSGDCompressor(LR_AGG), EFSignSGDMemory(LR_MEM), 1))]
    for a, b in pairs:
        for s in range(3):
            g = torch.from_numpy(_inputs(n, "normal", 90 + s)[1].copy()).to(DEV)
            oa, ob = a.step(g, "w"), b.step(g, "w")
            assert oa.dtype == F32 and torch.equal(oa.view(torch.int32), ob.view(torch.int32)), s
            for state in ("residuals", "momentums"):
                for owner_a, owner_b in ((a.memory, b.memory), (a.compressor, b.compressor)):
                    if hasattr(owner_a, state):
                        assert torch.equal(getattr(owner_a, state)["w"].view(torch.int32),
                                           getattr(owner_b, state)["w"].view(torch.int32)), (s, state)
            del oa, ob


def test_float16_is_still_refused():
    h = torch.ones(4096, dtype=torch.float16, device=DEV)
    for kind in ("u8", "bits", "signum", "ef"):
        comm = _comm(kind)
        with pytest.raises(TypeError):
            comm.step(h, "w")
        with pytest.raises(TypeError):
            comm.compressor.compress(h, "w")


# ------------------------------------------------------------------------------- world 2
W2_SIZES = (5003, (1 << 20) + 7)
W2_KINDS = ("u8", "bits", "signum", "ef")


def _w2_grad(n, rank, s):
    g = np.random.default_rng(9000 + 10 * rank + s + n % 1000).standard_normal(n).astype(np.float32)
    return torch.from_numpy(g).to(BF16)


def _w2_worker(rank, path, outdir):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=2)
    torch.cuda.set_device(0)
    from grace_amd import ops
    means, real = [], ops.efsign_step

    def wrapped(*a, **kw):
        r = real(*a, **kw)
        means.append(r[0])
        return r
    ops.efsign_step = wrapped
    res = {}
    for n in W2_SIZES:
        for kind in W2_KINDS:
            comm = _comm(kind, 2)
            for s in range(2):
                out = comm.step(_w2_grad(n, rank, s).to(DEV), "w")
                assert out.dtype == BF16 and out.shape == (n,)
                res[f"{n}_{kind}_out{s}"] = out.view(torch.int16).cpu().numpy()
                if kind == "ef":
                    assert comm.memory.residuals["w"].dtype == F32
                    res[f"{n}_ef_res{s}"] = comm.memory.residuals["w"].cpu().numpy()
                    res[f"{n}_ef_mean{s}"] = means[-1].cpu().numpy()
                if kind == "signum":
                    assert comm.compressor.momentums["w"].dtype == F32
                    res[f"{n}_signum_m{s}"] = comm.compressor.momentums["w"].cpu().numpy()
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


def test_bf16_steps_world2():
    """Two gloo processes on one device, two steps per class and size.  Expected: the majority of the
    two ranks' codes (signSGD on both wires, Signum on its momentum); for EF-signSGD each rank's util
    step with the mean that rank's device used, then ((0 + m_0 d_0) + m_1 d_1) / lr_agg narrowed
    once.  Both ranks hold the same bytes."""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_w2_worker, args=(os.path.join(tmp, "rdv"), tmp), nprocs=2, join=True)
        zs = [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(2)]
    for n in W2_SIZES:
        res, mom = [None, None], [None, None]
        for s in range(2):
            ups = [_w2_grad(n, r, s).float().numpy() for r in range(2)]
            for kind in W2_KINDS:
                assert np.array_equal(zs[0][f"{n}_{kind}_out{s}"], zs[1][f"{n}_{kind}_out{s}"]), (n, kind, s)
            vote = _pm1_bits(O.sign_aggregate([O.sign_decode(O.sign_encode(u)) for u in ups]) > 0)
            for wire in ("u8", "bits"):
                assert np.array_equal(zs[0][f"{n}_{wire}_out{s}"].view(np.uint16), vote), (n, wire, s)
            mom = [O.signum_momentum(ups[r], mom[r], 0.9) for r in range(2)]
            for r in range(2):
                assert np.array_equal(zs[r][f"{n}_signum_m{s}"].view(np.uint32), mom[r].view(np.uint32)), (n, s, r)
            vote = _pm1_bits(O.sign_aggregate([O.sign_decode(O.sign_encode(m)) for m in mom]) > 0)
            assert np.array_equal(zs[0][f"{n}_signum_out{s}"].view(np.uint16), vote), (n, s)
            means, codes = [], []
            for r in range(2):
                m = zs[r][f"{n}_ef_mean{s}"]
                t, c, _, res[r], _ = U.ef_step(ups[r], res[r], LR_MEM, m)
                assert _ulps(m[0], U.exact_mean(t)) <= 2, (n, s, r)
                assert U.same_bits_nan(zs[r][f"{n}_ef_res{s}"], res[r]), (n, s, r)
                means.append(m)
                codes.append(c)
            exp = U.ef_decode_aggregate(np.concatenate(means), np.concatenate(codes), 2, n, LR_AGG)
            check_dense(torch.from_numpy(zs[0][f"{n}_ef_out{s}"]).view(BF16), exp)
