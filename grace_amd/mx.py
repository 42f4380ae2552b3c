"""The OCP Microscaling (MX) formats as a gradient codec: blocks of 32 elements share one power-of-two scale
byte (E8M0, the floor rule of the OCP specification) and every element is an FP8 (``fp8_e4m3``, ``fp8_e5m2``),
FP6 (``fp6_e2m3``, ``fp6_e3m2``) or FP4 (``fp4_e2m1``) code: 8.25, 6.25 or 4.25 bits an element on the wire,
the same for a float32 and a bfloat16 gradient.  ``rounding="nearest"`` is deterministic (ties to the even
code); ``"stochastic"`` rounds up with the probability of the remainder, so the decoded gradient is unbiased
below the format's saturation point; its seed is drawn per (rank, name, step) as QSGD's is.  Stateless, fixed
rate: the payload's size depends on n and the format alone, so the exchange is one all-gather.  The arithmetic
and the wire are stated in include/grace_hip_mx.h.  The reference has no such codec.

``Allgather(MXCompressor(...), NoneMemory(), W).step`` on a CUDA float32 or bfloat16 tensor is fused at every
world size (one launch at world 1: neither codes nor scales reach memory) and returns the gradient's dtype.
``compress`` / ``decompress`` by hand, and so ResidualMemory, take float32; bfloat16 there and float16 anywhere
raise TypeError.  Blocks are counted from element 0 of the tensor handed in.  Not served: AllToAll (it raises
NotImplementedError), a fused ResidualMemory step, the sharded engines and the Horovod optimizer path.

``grace_from_params`` below is grace_amd.adaq's (and so grace_amd.dist's) with the key ``'mx'`` and its optional
``format`` and ``rounding`` added; every other params dict is handed on unchanged.
"""
import torch

from grace_amd import ops
from grace_amd.dist import Compressor
from grace_amd.dist.communicator.allgather import Allgather, _gather_flat
from grace_amd.dist.memory.none import NoneMemory


class MXCompressor(Compressor):

    def __init__(self, format="fp8_e4m3", rounding="nearest"):
        super().__init__(tensors_size_are_same=True)
        ops._mx_format(format, "MXCompressor")
        ops._mx_rounding(rounding, "MXCompressor")
        self.format = format
        self.rounding = rounding
        self._step = 0

    def _seed(self, name):
        self._step += 1
        if self.rounding == "nearest":
            return 0
        return ops.step_seed("mx", ops.rank_of_process(), name, self._step)

    def compress(self, tensor, name):
        payload = ops.mx_compress(ops.dev_f32(tensor), self.format, self.rounding, seed=self._seed(name))
        return [payload], (tensor.dtype, tensor.size())

    def decompress(self, tensor_compressed, ctx):
        dtype, shape = ctx
        return ops.mx_decode_aggregate(tensor_compressed[0], 1, shape.numel(), self.format,
                                       out_dtype=dtype).view(shape)

    def decode_aggregate_gathered(self, gathered, ctx, world_size):
        if not gathered[0].is_cuda:
            return None
        dtype, shape = ctx
        return ops.mx_decode_aggregate(gathered[0], world_size, shape.numel(), self.format,
                                       divisor=world_size if self.average else 1.0, out_dtype=dtype).view(shape)

    def fused_step(self, communicator, tensor, name):
        if communicator.__class__.__name__ == "AllToAll":
            raise NotImplementedError("MXCompressor: AllToAll is not served (the blocks do not split by rank)")
        if not (communicator.__class__ is Allgather and communicator.memory.__class__ is NoneMemory
                and isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype in (ops.F32, ops.BF16)):
            return None
        world = int(communicator.world_size)
        seed = self._seed(name)
        if world == 1:
            return ops.mx_step_w1(tensor, self.format, self.rounding, seed=seed)
        g = ops.dev_grad(tensor)
        gathered = _gather_flat(ops.mx_compress(g, self.format, self.rounding, seed=seed), world)
        return self.decode_aggregate_gathered([gathered], (g.dtype, tensor.shape), world)


def grace_from_params(params):
    """grace_amd.adaq.grace_from_params, plus ``'compressor': 'mx'`` with the optional keys ``format``
    ('fp8_e4m3') and ``rounding`` ('nearest'); memory and communicator as there."""
    from grace_amd.adaq import grace_from_params as base_from_params
    if params.get('compressor', 'none') != 'mx':
        return base_from_params(params)
    compressor = MXCompressor(params.get('format', 'fp8_e4m3'), params.get('rounding', 'nearest'))
    comm = base_from_params({**params, 'compressor': 'none'})   # the memory and the communicator
    comm.compressor = compressor
    return comm
