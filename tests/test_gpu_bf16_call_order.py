"""The bf16 stand-in engines (grace_amd.topk_bf16, sharded_bf16, segmented_bf16) make their parents'
native calls in their parents' order.

Bit-equal results do not pin that: two launches swapped, or one made twice, can give the same bits.
So ``_lib.call`` is wrapped with a pass-through that records the entry-point names (calls that go
through ``_lib.fn`` are not seen), and three world-1 steps of one name are run:

  * a float32 input through the stand-in class gives the parent class's sequence;
  * a bfloat16 input gives the literal sequence written here.

Whether a stand-in repeats its parent's step body or overrides pieces of it, this is what tells
when the two stop making the same calls.

Every run is made twice and the second is the one recorded, so what a process does once (a status
word, a workspace query) is not in the sequence.  The shapes are the smallest the other bf16 test
files use to reach every launch branch.  Then one name is stepped bf16, f32, bf16: the residual is
the all-f32 run's, bit for bit, and each result has its input's dtype (the sharded engine has that
test in tests/test_gpu_sharded_bf16.py).
"""
import pytest
import torch

from tests.test_gpu_segmented_bf16 import EDGE_SIZES, _edge_case, _flat_bf16
from tests.test_gpu_topk_bf16 import _inputs

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
F32 = torch.float32
RATIO = 0.01
STEPS = 3


@pytest.fixture
def trace(monkeypatch):
    """trace(run) -> the names run() hands to _lib.call, on its second execution."""
    from grace_amd import _lib
    names = []
    real = _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", recording)

    def trace(run):
        run()
        del names[:]
        run()
        return list(names)
    return trace


def _grad(n, step, dtype):
    b, up = _inputs(n, "normal", 700 + step)
    return b.cuda() if dtype == BF16 else torch.from_numpy(up.copy()).cuda()


def _same_i32(a, b):
    return a.dtype == b.dtype == F32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------- Allgather top-k
def _allgather_steps(compressor_cls, memory_cls, n, dtype):
    from grace_amd.dist.communicator.allgather import Allgather

    def run():
        comm = Allgather(compressor_cls(RATIO), memory_cls(), 1)
        for s in range(STEPS):
            comm.step(_grad(n, s, dtype), "w")
        torch.cuda.synchronize()
    return run


TOPK_BF16_CALLS = {
    "ResidualMemory": ["grace_topk_residual_step_bf16"] * STEPS,
    "NoneMemory": ["grace_topk_step_dense_bf16"] * STEPS,
}


@pytest.mark.parametrize("n", [9001, 40003])      # one workgroup / the multi-workgroup pass
@pytest.mark.parametrize("memory", ["ResidualMemory", "NoneMemory"])
def test_allgather_topk_call_order(trace, memory, n):
    from grace_amd.dist.compressor.topk import TopKCompressor as Parent
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    from grace_amd.topk_bf16 import TopKCompressor
    mem = {"ResidualMemory": ResidualMemory, "NoneMemory": NoneMemory}[memory]
    parent = trace(_allgather_steps(Parent, mem, n, F32))
    ours = trace(_allgather_steps(TopKCompressor, mem, n, F32))
    print("f32", memory, n, ours)
    assert parent and ours == parent
    got = trace(_allgather_steps(TopKCompressor, mem, n, BF16))
    print("bf16", memory, n, got)
    assert got == TOPK_BF16_CALLS[memory]


# ------------------------------------------------------------------------------- sharded
def _sharded_steps(cls, dtype):
    def run():
        eng = cls(RATIO)
        for s in range(STEPS):
            eng.step(_grad(40003, s, dtype), "b")     # the result is dropped: the next step takes it back
        eng.check()
    return run


SHARDED_BF16_CALLS = (["grace_fill_bf16", "grace_topk_residual_step_swap_bf16", "grace_shard_select_bf16"]
                      + ["grace_shard_clear_bf16", "grace_topk_residual_step_swap_bf16", "grace_shard_select_bf16"]
                      * (STEPS - 1))


def test_sharded_call_order(trace):
    from grace_amd.dist.sharded import ShardedTopK as Parent
    from grace_amd.sharded_bf16 import ShardedTopK
    parent = trace(_sharded_steps(Parent, F32))
    ours = trace(_sharded_steps(ShardedTopK, F32))
    print("f32 sharded", ours)
    assert parent and ours == parent
    assert "grace_shard_clear" in parent              # the recycle-and-clear branch ran
    got = trace(_sharded_steps(ShardedTopK, BF16))
    print("bf16 sharded", got)
    assert got == SHARDED_BF16_CALLS


# ------------------------------------------------------------------------------- segmented
def _edge_flat(step, dtype):
    flat = _flat_bf16(_edge_case()[0][step])
    return flat if dtype == BF16 else flat.float()


def _segmented_steps(cls, dtype):
    def run():
        eng = cls(RATIO)
        for s in range(STEPS):
            eng.step(_edge_flat(s, dtype), EDGE_SIZES)
        torch.cuda.synchronize()
    return run


SEGMENTED_BF16_CALLS = ["grace_topk_segmented_step_bf16"] * STEPS


def test_segmented_call_order(trace):
    from grace_amd.dist.segmented import SegmentedTopK as Parent
    from grace_amd.segmented_bf16 import SegmentedTopK
    parent = trace(_segmented_steps(Parent, F32))
    ours = trace(_segmented_steps(SegmentedTopK, F32))
    print("f32 segmented", ours)
    assert parent and ours == parent
    got = trace(_segmented_steps(SegmentedTopK, BF16))
    print("bf16 segmented", got)
    assert got == SEGMENTED_BF16_CALLS


# ------------------------------------------------------------------------------- dtype switch
SWITCH = (BF16, F32, BF16)


def test_allgather_topk_dtype_switch_on_one_name():
    """bf16, f32, bf16 (the existing test runs f32, bf16, f32: there the parent writes the name's
    first residual; here the stand-in does and the parent has to take it)."""
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.topk import TopKCompressor as Parent
    from grace_amd.dist.memory.residual import ResidualMemory
    from grace_amd.topk_bf16 import TopKCompressor
    n = 40003
    comm, ref = Allgather(TopKCompressor(RATIO), ResidualMemory(), 1), Allgather(Parent(RATIO), ResidualMemory(), 1)
    for s, dtype in enumerate(SWITCH):
        out = comm.step(_grad(n, s, dtype), "w")
        ref.step(_grad(n, s, F32), "w")
        assert out.dtype == dtype, s
        assert _same_i32(comm.memory.residuals["w"], ref.memory.residuals["w"]), s


def test_segmented_dtype_switch_on_one_name():
    from grace_amd.dist.segmented import SegmentedTopK as Parent
    from grace_amd.segmented_bf16 import SegmentedTopK
    eng, ref = SegmentedTopK(RATIO), Parent(RATIO)
    for s, dtype in enumerate(SWITCH):
        out = eng.step(_edge_flat(s, dtype), EDGE_SIZES, "w")
        ref.step(_edge_flat(s, F32), EDGE_SIZES, "w")
        assert out.dtype == dtype, s
        assert _same_i32(eng.residuals["w"], ref.residuals["w"]), s
