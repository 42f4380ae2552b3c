"""The quantisers (grace_amd/csrc/quant.hip) on the two size-conditional kernel families that the
ResNet-50 set never reaches, and the pipelined encoder's int8 shortcut at its magnitude edges.

Part A, more than kSegLds = 512 segments: the offset tables stay in global memory, so QSGD runs
qsgd_encode_kernel / qsgd_decode_kernel<.., B128 = true> and TernGrad tern_stats / tern_encode on a
global SegView and tern_decode_kernel with tern_decode_slow; 512 segments is the full LDS table.

Part B, more than 262,144 buckets of 128: every capped row kernel gives a workgroup more than one
trip (the pipelined encoder refills tile A, the decoders carry their segment cursor), and the
general decoder runs a second kDecRound round past 4096 * 4096 elements.

Part C, the pipelined encoder's int8 shortcut where 1 / norm * q overflows, where the sum of squares
overflows or underflows, and where a level sits at q and rounds up to q + 1.

Everything is compared with the CPU oracle per segment: codes bit-exact given the injected (or
restated, tests/device_rng.py) uniforms and the device's scales, decodes bit-exact given codes and
scales, scales within the suite's ulp bounds of the oracle's."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from grace_amd import _lib, ops
from oracle import grace_oracle as O
from tests.device_rng import qsgd_bucket128_uniforms
from tests.golden_util import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
QV = [(127, 0), (255, 0), (127, 1)]


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # (a copy: the shared inputs are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def norms_close(dev, ref, ulps):
    """Scales within `ulps` of the reference where it is finite, the same bits where it is inf / NaN."""
    dev, ref = np.asarray(dev, dtype=F32), np.asarray(ref, dtype=F32)
    fin = np.isfinite(ref)
    return same_bits(np.isnan(dev[~fin]), np.isnan(ref[~fin])) and \
        np.array_equal(dev[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]) and \
        ops.isclose_f32_ulps(dev[fin], ref[fin], ulps)


def bucket_index(sizes, bucket):
    """The norm index of every element of a segmented buffer (numpy; small layouts only)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    sub = np.concatenate([[0], np.cumsum(-(-sizes // bucket))])[:-1]
    seg = np.repeat(np.arange(len(sizes)), sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    return sub[seg] + (np.arange(int(sizes.sum())) - off[seg]) // bucket


def decode_formula(codes, norms, bidx, q, variant=0):
    """(norm / q) * code in f32, one rounding per operation (qsgd.py:44-49 = O.qsgd_decode); variant 1
    decodes the codeword -128 to NaN."""
    with np.errstate(invalid="ignore"):
        d = ((norms[bidx] / F32(q)).astype(F32) * codes.astype(F32)).astype(F32)
    if variant == 1:
        d[codes == -128] = np.nan
    return d


# ================================================================================================
# Part A: the segment-count limit
PINNED = [1, 2, 3, 127, 128, 129, 256, 4099]
TERN_UNIT = 16384


@functools.lru_cache(maxsize=None)
def seg_layout(nseg, odd):
    """nseg sizes drawn from [1, 600] with PINNED at seeded places (4099 last), n = 4 k (odd=False: a
    code stride that is a multiple of 4, the decoders' `vec` loads at world > 1) or n odd; the
    700-segment layout also holds one segment longer than a TernGrad unit.  Returns (sizes, x, u): N(0, 0.01^2) data and
    uniforms, shared (read-only) by the tests."""
    rng = np.random.default_rng(7000 + nseg)
    sizes = rng.integers(1, 601, size=nseg)
    place = rng.choice(nseg - 1, len(PINNED) + 1, replace=False)
    sizes[place[:len(PINNED) - 1]] = PINNED[:-1]
    sizes[-1] = PINNED[-1]   # 33 buckets last: every segment cursor has to advance into the final segment
    if nseg == 700:
        sizes[place[-2]] = 2 * TERN_UNIT + 77
    adj = place[-1]
    rest = int(sizes.sum() - sizes[adj])
    sizes[adj] = 300 + ((-(rest + 300)) % 4 if not odd else (rest + 300 + 1) % 2)
    n = int(sizes.sum())
    assert (n % 2 == 1) if odd else (n % 4 == 0)
    assert set(PINNED) <= set(sizes.tolist()) and sizes.min() >= 1
    rng = np.random.default_rng(nseg + odd)
    x = (rng.standard_normal(n) * 0.01).astype(F32)
    u = rng.random(n, dtype=F32)
    x.setflags(write=False)
    u.setflags(write=False)
    return tuple(int(s) for s in sizes), x, u


def with_specials(sizes, x):
    """Variant 1's inputs: a NaN, a +inf and a -inf in different segments and one all-zero bucket."""
    x = x.copy()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    big = int(np.flatnonzero(np.asarray(sizes) == 4099)[0])
    x[offs[big] + 1024:offs[big] + 1152] = 0.0
    picks = [s for s in (5, len(sizes) // 2, len(sizes) - 2) if s != big]
    assert len(picks) == 3
    for s, v in zip(picks, (np.nan, np.inf, -np.inf)):
        x[offs[s] + sizes[s] // 2] = v
    return x


def check_qsgd_segments(x, u, sizes, q, bucket, variant, codes, norms, dec):
    """Per segment against the oracle, as test_segmented_qsgd_bucket_and_code_variants (variant 0)
    and test_qsgd_cuda_variant_vs_oracle_with_specials (variant 1) do."""
    cn, nn, d = _np(codes), _np(norms), _np(dec)
    ref_norms = []
    off = noff = 0
    for i, n in enumerate(sizes):
        nb = -(-n // bucket)
        xs, us, dn = x[off:off + n], u[off:off + n], nn[noff:noff + nb]
        if variant == 0:
            ref_norms.append(O.qsgd_norms(xs, bucket))
            exp_c, _ = O.qsgd_compress(xs, us, q, bucket, norms=dn)
            assert same_bits(cn[off:off + n], exp_c), (i, n, q, bucket)
            assert same_bits(d[off:off + n], O.qsgd_decode(exp_c, dn, q, bucket, n)), (i, n, q, bucket)
        else:
            ref_norms.append(O.qsgd_cuda_compress(xs, us, q, bucket)[1].astype(F32))
            exp_c, _ = O.qsgd_cuda_compress(xs, us, q, bucket, norms=dn)
            assert np.array_equal(cn[off:off + n], exp_c), (i, n)
            assert np.all(exp_c[~np.isfinite(xs)] == -128)
            ds = d[off:off + n]
            assert np.all(np.isnan(ds[exp_c == -128]))
            ok = exp_c != -128
            exp_d = decode_formula(exp_c, dn, np.arange(n) // bucket, q)
            assert same_bits(ds[ok], exp_d[ok]), (i, n)
        off += n
        noff += nb
    assert noff == nn.size and off == cn.size
    # f32 norms of N(0, 0.01^2) data: the suite's 4 ulp; variant 1's f64 norms: 1 ulp
    assert norms_close(nn, np.concatenate(ref_norms), 4 if variant == 0 else 1)


@pytest.mark.parametrize("q,variant", QV)
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("nseg", [512, 513, 700])
def test_segments_qsgd128_injected_uniforms(nseg, odd, q, variant):
    """Bucket 128 with an injected stream: qsgd_encode128_kernel / qsgd_decode_bkt_kernel on the full
    LDS table at 512 segments, qsgd_encode_kernel (bucket <= 128 branch) and
    qsgd_decode_kernel<.., B128> on global tables beyond."""
    sizes, x, u = seg_layout(nseg, odd)
    if variant == 1:
        x = with_specials(sizes, x)
    codes, norms = ops.qsgd_compress(_t(x), q, 128, sizes=sizes, variant=variant, u=_t(u))
    dec = ops.qsgd_decompress(codes, norms, q, 128, x.size, sizes=sizes, variant=variant)
    check_qsgd_segments(x, u, sizes, q, 128, variant, codes, norms, dec)
    if variant == 1:
        assert (_np(codes) == -128).sum() >= 3 and np.isnan(_np(dec)).sum() >= 3


@pytest.mark.parametrize("q,variant", QV)
@pytest.mark.parametrize("nseg,odd", [(512, True), (513, False), (513, True), (700, False), (700, True)])
def test_segments_qsgd128_device_generator(nseg, odd, q, variant):
    """seed= and no u: beyond 512 segments qsgd_encode_kernel draws uniform01x4(seed, e) itself, at
    512 the pipelined kernel runs on a full LDS table.  Bit for bit the codes of the same call fed
    the restated draws."""
    sizes, x, _ = seg_layout(nseg, odd)
    if variant == 1:
        x = with_specials(sizes, x)
    seed = 0xBEEF00 + nseg + q
    u = qsgd_bucket128_uniforms(seed, sizes)
    codes, norms = ops.qsgd_compress(_t(x), q, 128, sizes=sizes, variant=variant, seed=seed)
    codes_u, norms_u = ops.qsgd_compress(_t(x), q, 128, sizes=sizes, variant=variant, u=_t(u))
    assert same_bits(_np(norms), _np(norms_u))
    assert same_bits(_np(codes), _np(codes_u))
    if nseg == 512:   # the pipelined kernel has no other oracle check at a full table
        dec = ops.qsgd_decompress(codes, norms, q, 128, x.size, sizes=sizes, variant=variant)
        check_qsgd_segments(x, u, sizes, q, 128, variant, codes, norms, dec)


@pytest.mark.parametrize("q", [127, 200])
@pytest.mark.parametrize("bucket", [37, 512])
def test_segments_qsgd_other_buckets(bucket, q):
    """700 segments at bucket 37 (a quarter-filled half-wave per bucket) and bucket 512 (the
    bucket > 128 loop with half_sum), int8 and fp16 codes; the general decoder with B128 = false."""
    sizes, x, u = seg_layout(700, True)
    codes, norms = ops.qsgd_compress(_t(x), q, bucket, sizes=sizes, u=_t(u))
    dec = ops.qsgd_decompress(codes, norms, q, bucket, x.size, sizes=sizes)
    check_qsgd_segments(x, u, sizes, q, bucket, 0, codes, norms, dec)


@pytest.mark.parametrize("sizes", [(1,), (129,), (64, 1, 129)], ids=lambda s: "n%d" % sum(s))
def test_qsgd_cuda_variant_other_bucket(sizes):
    """Variant 1 away from bucket 128 (bucket 100, 64 levels): qsgd_encode_kernel<int8, 1> on a
    generic bucket and qsgd_decode_kernel<int8, 1, B128 = false>, the one arm of the launchers'
    (code type, variant) choice that no other test reaches.  Codes, norms and the dense result are
    written in front of a canary that has to survive."""
    from grace_amd import _lib
    q, bucket, guard = 64, 100, 64
    n = sum(sizes)
    rng = np.random.default_rng(6400 + n)
    x = (rng.standard_normal(n) * 0.01).astype(F32)
    u = rng.random(n, dtype=F32)
    if n > 100:
        x[[3, n - 2]] = [np.nan, -np.inf]     # the first and the last bucket hold a codeword -128
    nb = sum(-(-s // bucket) for s in sizes)
    cbuf = torch.full((n + guard,), 0x5A, dtype=torch.int8, device=DEV)
    nbuf = torch.full((nb + guard,), -7.0, dtype=torch.float32, device=DEV)
    dbuf = torch.full((n + guard,), -7.0, dtype=torch.float32, device=DEV)
    codes, norms = ops.qsgd_compress(_t(x), q, bucket, sizes=list(sizes), variant=1, u=_t(u),
                                     codes_out=cbuf[:n], norms_out=nbuf[:nb])
    seg_off, bkt_off, nb_t = ops.seg_tables(list(sizes), bucket, codes.device)
    assert nb_t == nb
    dec = dbuf[:n]
    _lib.call("grace_qsgd_decompress", ops._p(codes), ops._p(norms), n, nb, 1, ops._p(seg_off), ops._p(bkt_off),
              len(sizes), n, q, bucket, 1, 0, 1.0, ops._p(dec), ops._stream())
    check_qsgd_segments(x, u, sizes, q, bucket, 1, codes, norms, dec)
    assert bool((cbuf[n:] == 0x5A).all()) and bool((nbuf[nb:] == -7.0).all()) and bool((dbuf[n:] == -7.0).all())
    if n > 100:
        assert (_np(codes) == -128).sum() == 2 and np.isnan(_np(dec)).sum() == 2


@pytest.mark.parametrize("q", [127, 255])
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("nseg", [512, 513, 700])
def test_segments_qsgd_decode_world3(nseg, odd, q):
    """Three payloads summed from 0 in rank order and divided by 3, int8 and fp16 codes, with a code
    stride that is (odd=False) and is not a multiple of 4."""
    sizes, x, u = seg_layout(nseg, odd)
    n = x.size
    cs, ns = [], []
    for w in range(3):
        xw = np.roll(x, 1000 * w) * F32(1 + w)
        c, nm = ops.qsgd_compress(_t(xw), q, 128, sizes=sizes, u=_t(np.roll(u, 77 * w)))
        cs.append(c)
        ns.append(nm)
    out = _np(ops.qsgd_decompress(torch.cat(cs), torch.cat(ns), q, 128, n, sizes=sizes, world=3, aggregate=True,
                                  divisor=3.0))
    bidx = bucket_index(sizes, 128)
    decs = [decode_formula(_np(c), _np(nm), bidx, q) for c, nm in zip(cs, ns)]
    exp = (O.python_sum(decs) / F32(3)).astype(F32)
    assert same_bits(out, exp)


def tern_expected_codes(x, u, scalar):
    """terngrad.py:14-24 given the scalar: scalar = min(max|x|, c), so |clamp(x, -c, c)| is
    min(|x|, scalar) whichever of the two the scalar is; code = 0 where u * scalar >= |clamp x|."""
    scalar = F32(scalar)
    absg = np.minimum(np.abs(x), scalar)
    rnd = (u * scalar).astype(F32)
    return np.where(rnd >= absg, 0, np.sign(x) * (scalar != 0)).astype(np.int8)


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("nseg", [512, 513, 700])
def test_segments_terngrad_compress(nseg, odd):
    """tern_stats_kernel / tern_encode_kernel on global tables (700: find_seg over the unit table
    with a three-unit segment): an injected clip gives the oracle's codes and scalars bit for bit;
    device statistics give scalars within 4 ulp and the codes that follow from the device's scalar."""
    sizes, x, u = seg_layout(nseg, odd)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    segs = [(x[offs[i]:offs[i + 1]], u[offs[i]:offs[i + 1]]) for i in range(nseg)]
    clips = np.array([O.terngrad_clip(xs) for xs, _ in segs], dtype=F32)
    exp = [O.terngrad_compress(xs, us, clip=c) for (xs, us), c in zip(segs, clips)]
    codes, scal = ops.terngrad_compress(_t(x), sizes=sizes, u=_t(u), clip=_t(clips))
    assert same_bits(_np(scal), np.concatenate([e[1] for e in exp]))
    assert np.array_equal(_np(codes), np.concatenate([e[0] for e in exp]))
    codes, scal = ops.terngrad_compress(_t(x), sizes=sizes, u=_t(u))
    s = _np(scal)
    assert ops.isclose_f32_ulps(s, np.concatenate([e[1] for e in exp]), 4)
    exp_c = np.concatenate([tern_expected_codes(xs, us, s[i]) for i, (xs, us) in enumerate(segs)])
    assert np.array_equal(_np(codes), exp_c)


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("nseg", [512, 513, 700])
def test_segments_terngrad_decode(nseg, odd, world):
    """tern_decode_row_kernel on the full LDS table at 512 segments, tern_decode_kernel with
    tern_decode_slow beyond; world 3 aggregates in rank order with both code strides."""
    sizes, x, _ = seg_layout(nseg, odd)
    n = x.size
    rng = np.random.default_rng(nseg + world)
    codes = rng.integers(-1, 2, size=world * n, dtype=np.int8)
    scal = rng.random(world * nseg, dtype=F32)
    out = _np(ops.terngrad_decompress(_t(codes), _t(scal), n, sizes=sizes, world=world, aggregate=world > 1,
                                      divisor=float(world)))
    seg = np.repeat(np.arange(nseg), sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    if world == 1:
        exp = np.concatenate([O.terngrad_decode(codes[offs[i]:offs[i + 1]], scal[i:i + 1]) for i in range(nseg)])
    else:
        decs = [codes[w * n:(w + 1) * n].astype(F32) * scal[w * nseg + seg] for w in range(world)]
        exp = (O.python_sum(decs) / F32(world)).astype(F32)
    assert same_bits(out, exp)


def test_segments_fused_step_refuses_513():
    """The fused world-1 step keeps its tables in LDS: 513 segments are a bad-arguments error before
    any launch (the output keeps its fill), and qsgd_step_w1_ok says so; 512 run."""
    s512, x512, _ = seg_layout(512, True)
    s513, x513, _ = seg_layout(513, True)
    assert ops.qsgd_step_w1_ok(s512, 128) and not ops.qsgd_step_w1_ok(s513, 128)
    xd = _t(x513)
    with pytest.raises(_lib.GraceNativeError, match="grace_qsgd_step_w1: bad arguments"):
        ops.qsgd_step_w1(xd, 127, sizes=s513, seed=3)
    seg_off, bkt_off, nb = ops.seg_tables(s513, 128, xd.device)
    out = torch.full((xd.numel(),), 7.0, device=DEV)
    with pytest.raises(_lib.GraceNativeError, match="grace_qsgd_step_w1: bad arguments"):
        _lib.call("grace_qsgd_step_w1", xd.data_ptr(), seg_off.data_ptr(), bkt_off.data_ptr(), len(s513), nb, 127, 0,
                  None, ops.seed64(3), out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert (_np(out) == 7.0).all()
    xd = _t(x512)
    codes, norms = ops.qsgd_compress(xd, 127, 128, sizes=s512, seed=3)
    dec = ops.qsgd_decompress(codes, norms, 127, 128, xd.numel(), sizes=s512)
    assert same_bits(_np(ops.qsgd_step_w1(xd, 127, sizes=s512, seed=3)), _np(dec))


# ================================================================================================
# Part B: the bucket-count limit
PATTERN = [128 * 2000,       # starts 16-B aligned
           128 * 1500 + 5,   # partial last bucket
           3,                # starts unaligned; the next segment starts at offset = 8 mod 16
           128 * 1500,       # whole buckets with base & 15 == 8: direct 4-B stores, not the staged 16-B ones
           128 * 900 + 2,    # partial last bucket
           128 * 40,         # base & 3 == 2: every bucket goes to the per-element loop after the pipeline
           6, 1,
           15]               # restores 16-B alignment for the next repetition
REPS = 50
SPOT_REPS = (REPS // 2, REPS - 1)   # the repetitions copied to the host for the oracle


def _kernel_const(name):
    """A `constexpr int` of quant.hip: the restated grid arithmetic below follows the source, so a
    changed cap fails the trip-count assertions instead of quietly making this a one-trip test."""
    src = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "quant.hip")
    with open(src) as f:
        m = re.search(r"constexpr int %s = (\d+);" % name, f.read())
    return int(m.group(1))


def _stream_grid(n_vec, block, cap):   # common.h stream_grid
    return min(cap, max(1, -(-n_vec // block)))


def _range_per(total, grid, step=16):   # block_range32: a workgroup's range, rounded up to 16 rows
    return -(-(-(-total // grid)) // step) * step


def row_kernel_ranges(n, nseg, nbuckets):
    """Buckets (chunks) per workgroup of the capped row kernels, restating qenc_pipe_grid and
    block_range32 with kQEncPipeGridCap, kQEncGridCap and kQGridCap: the pipelined encoder, the
    non-pipelined / fused encoder, the bucket decoder and TernGrad's row decoder.  (qenc_pipe_grid's
    `need` term, the LDS bucket table outgrowing kQBkMax, first matters above about 4.06 M buckets,
    a 2 GB input: restated, not exercised.)"""
    rows_per_iter = _kernel_const("kQNB") * _kernel_const("kQBlock") // 16
    need = -(-nbuckets // (_kernel_const("kQBkMax") - 32))
    pipe = max(_stream_grid(nbuckets, rows_per_iter, _kernel_const("kQEncPipeGridCap")), need)
    enc = _stream_grid(nbuckets, rows_per_iter, _kernel_const("kQEncGridCap"))
    dec = _stream_grid((n + 127) // 128 + nseg, rows_per_iter, _kernel_const("kQGridCap"))
    tern = _stream_grid((n + 127) // 128, rows_per_iter, _kernel_const("kQGridCap"))
    return (_range_per(nbuckets, pipe), _range_per(nbuckets, enc), _range_per(nbuckets, dec),
            _range_per((n + 127) // 128, tern))


class BigLayout:
    """REPS repetitions of PATTERN: 450 segments, 297,350 buckets, 38.0 M elements, with its bucket
    table (numpy, per bucket), its per-element index tables (device) and the data (device)."""

    def __init__(self):
        self.sizes = PATTERN * REPS
        sz = np.asarray(self.sizes, dtype=np.int64)
        self.nseg, self.n = len(sz), int(sz.sum())
        self.off = np.concatenate([[0], np.cumsum(sz)])
        self.sub = np.concatenate([[0], np.cumsum((sz + 127) // 128)])
        self.nb = int(self.sub[-1])
        self.bseg = np.repeat(np.arange(self.nseg), (sz + 127) // 128)          # bucket -> segment
        self.base = self.off[self.bseg] + (np.arange(self.nb) - self.sub[self.bseg]) * 128
        whole = self.base + 128 <= self.off[self.bseg + 1]
        self.full = whole & (self.base % 4 == 0)       # the pipeline's buckets; the rest are encoded after it
        self.aligned16 = whole & (self.base % 16 == 0)
        self.per_pipe, self.per_enc, self.per_dec, self.per_tern = row_kernel_ranges(self.n, self.nseg, self.nb)
        self.jrel = np.arange(self.nb) % self.per_pipe                          # position in its workgroup's range
        g = torch.Generator(device=DEV)
        g.manual_seed(20240)
        self.x = torch.randn(self.n, generator=g, device=DEV) * 0.01
        self.x2 = torch.randn(self.n, generator=g, device=DEV) * 0.01
        sizes_d = torch.tensor(self.sizes, device=DEV)
        self.seg_d = torch.repeat_interleave(torch.arange(self.nseg, device=DEV), sizes_d)   # element -> segment
        off_d, sub_d = torch.from_numpy(self.off).to(DEV), torch.from_numpy(self.sub).to(DEV)
        self.bidx_d = sub_d[self.seg_d] + (torch.arange(self.n, device=DEV) - off_d[self.seg_d]) // 128
        self.spot = [s for r in SPOT_REPS for s in range(r * len(PATTERN), (r + 1) * len(PATTERN))]

    def planted(self):
        """Four whole aligned buckets of the middle spot-check repetition at range-relative positions
        >= 32 (pipeline stages past the first), one each side of position 64: (bucket, what)."""
        lo, hi = self.sub[SPOT_REPS[0] * len(PATTERN)], self.sub[(SPOT_REPS[0] + 1) * len(PATTERN)]
        inrep = (np.arange(self.nb) >= lo) & (np.arange(self.nb) < hi)
        pick = lambda m: int(np.flatnonzero(inrep & m)[0])   # noqa: E731
        a16, j = self.aligned16, self.jrel
        a8 = self.full & (self.base % 16 == 8)
        return [(pick(a16 & (j >= 32) & (j < 48)), "zero"), (pick(a16 & (j >= 64)), "+inf"),
                (pick(a16 & (j >= 48) & (j < 64)), "nan"), (pick(a8 & (j >= 64)), "-inf")]


@pytest.fixture(scope="module")
def big():
    lay = BigLayout()
    yield lay
    del lay
    torch.cuda.empty_cache()


def test_big_layout_trip_counts(big):
    """The conditions that make part B a multi-trip test, from the restated range arithmetic."""
    assert big.nseg <= _kernel_const("kSegLds") and 262144 < big.nb <= 327680
    assert big.per_pipe > 64, big.per_pipe     # the pipelined encoder refills tile A
    assert big.per_enc > 64, big.per_enc       # the non-pipelined / fused encoder: third trip
    assert big.per_dec > 32, big.per_dec       # the bucket decoder carries its cursor
    assert big.per_tern > 32, big.per_tern
    odd = ~big.full
    assert (odd & (big.jrel >= 64)).any()
    assert (odd & (big.jrel % 32 // 16 == 0)).any() and (odd & (big.jrel % 32 // 16 == 1)).any()
    for b, _ in big.planted():
        assert big.full[b] and big.jrel[b] >= 32
    assert len({b for b, _ in big.planted()}) == 4


def dev_same(a, b):
    """Bitwise equal f32 device tensors, NaN equal to NaN."""
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def dev_decode_formula(big, codes, norms, q, variant):
    """(norms[bucket_of_element] / q) * code on the device.  The per-bucket quotient is taken in
    numpy (correctly rounded: torch may divide by a scalar through its reciprocal), the per-element
    product is one f32 multiply."""
    scale = _t((_np(norms) / F32(q)).astype(F32))
    d = scale[big.bidx_d] * codes.float()
    if variant == 1:
        d = torch.where(codes == -128, torch.full_like(d, float("nan")), d)
    return d


@pytest.mark.parametrize("q,variant", QV)
def test_big_qsgd_bucket128(big, q, variant):
    """80 buckets per workgroup in the encoders, 48 in the bucket decoder.  The pipelined encoder
    against the non-pipelined one over the whole array, the oracle on two repetitions of the
    pattern (the planted zero / inf / NaN buckets are in the first), the decoder at world 1 and 2
    against its formula over the whole array and the oracle on the same slices, the fused step."""
    assert big.per_pipe > 64 and big.per_dec > 32
    x = big.x
    seed = 0x5EED00 + q + variant
    if variant == 0:
        x = x.clone()
        for b, what in big.planted():
            lo = int(big.base[b])
            if what == "zero":
                x[lo:lo + 128] = 0.0
            else:
                x[lo + 37] = {"+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan")}[what]
    as_int = (lambda c: c) if q < 128 else (lambda c: c.view(torch.int16))
    # 1. pipelined == non-pipelined, every code and norm
    codes, norms = ops.qsgd_compress(x, q, 128, sizes=big.sizes, variant=variant, seed=seed)
    _, norms_ref = ops.qsgd_compress(x, q, 128, sizes=big.sizes, variant=variant, u=torch.zeros_like(x))
    assert torch.equal(norms.view(torch.int32), norms_ref.view(torch.int32))
    codes_ref, _ = ops.qsgd_compress(x, q, 128, sizes=big.sizes, variant=variant, seed=seed, norms_in=norms)
    assert torch.equal(as_int(codes), as_int(codes_ref))
    del codes_ref, norms_ref
    # 3. the bucket decoder against its formula, world 1 and world 2
    dec = ops.qsgd_decompress(codes, norms, q, 128, big.n, sizes=big.sizes, variant=variant)
    d0 = dev_decode_formula(big, codes, norms, q, variant)
    assert dev_same(dec, d0)
    codes2, norms2 = ops.qsgd_compress(big.x2, q, 128, sizes=big.sizes, variant=variant, seed=seed + 1)
    dec2 = ops.qsgd_decompress(torch.cat([codes, codes2]), torch.cat([norms, norms2]), q, 128, big.n, sizes=big.sizes,
                               variant=variant, world=2, aggregate=True, divisor=2.0)
    d1 = dev_decode_formula(big, codes2, norms2, q, variant)
    assert dev_same(dec2, ((0.0 + d0) + d1) / 2.0)   # (/ 2 and * 0.5 round alike)
    del d0, d1
    # 4. the fused world-1 step: the non-pipelined kernel past its second trip
    assert dev_same(ops.qsgd_step_w1(x, q, sizes=big.sizes, variant=variant, seed=seed), dec)
    # 2. (and 3.) the oracle on the spot-check segments
    nn, nn2 = _np(norms), _np(norms2)
    ref_norms, got_norms = [], []
    for s in big.spot:
        lo, hi, blo, bhi = int(big.off[s]), int(big.off[s + 1]), int(big.sub[s]), int(big.sub[s + 1])
        xs, cs, dn = _np(x[lo:hi]), _np(codes[lo:hi]), nn[blo:bhi]
        us = qsgd_bucket128_uniforms(seed, big.sizes, segs=(s, s + 1))
        bi = np.arange(hi - lo) // 128
        if variant == 0:
            ref_norms.append(O.qsgd_norms(xs, 128))
            exp_c, _ = O.qsgd_compress(xs, us, q, 128, norms=dn)
            assert same_bits(cs, exp_c), s
            with np.errstate(invalid="ignore"):   # (an inf norm times the code 0)
                exp_d = O.qsgd_decode(exp_c, dn, q, 128, hi - lo)
        else:
            ref_norms.append(O.qsgd_cuda_compress(xs, us, q, 128)[1].astype(F32))
            exp_c, _ = O.qsgd_cuda_compress(xs, us, q, 128, norms=dn)
            assert np.array_equal(cs, exp_c), s
            exp_d = decode_formula(exp_c, dn, bi, q, 1)
        got_norms.append(dn)
        assert same_bits(np.isnan(exp_d), np.isnan(_np(dec[lo:hi]))), s
        ok = ~np.isnan(exp_d)
        assert same_bits(_np(dec[lo:hi])[ok], exp_d[ok]), s
        with np.errstate(invalid="ignore"):
            exp_2 = (O.python_sum([exp_d, decode_formula(_np(codes2[lo:hi]), nn2[blo:bhi], bi, q, variant)])
                     / F32(2)).astype(F32)
        assert same_bits(_np(dec2[lo:hi])[ok], exp_2[ok]), s
    assert norms_close(np.concatenate(got_norms), np.concatenate(ref_norms), 4 if variant == 0 else 1)
    if variant == 0:   # the planted buckets reached the checks above
        for b, what in big.planted():
            assert big.bseg[b] in big.spot
            assert {"zero": nn[b] == 0, "nan": np.isnan(nn[b])}.get(what, np.isinf(nn[b])), (b, what)


def test_big_terngrad_decode(big):
    """tern_decode_row_kernel with 48 chunks per workgroup: the cursor carried over a second trip.
    The whole array against code * scalar of the element's segment, the spot-check segments against
    the oracle, at world 1 and at world 2 aggregated."""
    assert big.per_tern > 32
    c0, s0 = ops.terngrad_compress(big.x, sizes=big.sizes, seed=11)
    c1, s1 = ops.terngrad_compress(big.x2, sizes=big.sizes, seed=12)
    dec = ops.terngrad_decompress(c0, s0, big.n, sizes=big.sizes)
    d0 = c0.float() * s0[big.seg_d]
    assert dev_same(dec, d0)
    dec2 = ops.terngrad_decompress(torch.cat([c0, c1]), torch.cat([s0, s1]), big.n, sizes=big.sizes, world=2,
                                   aggregate=True, divisor=2.0)
    assert dev_same(dec2, ((0.0 + d0) + c1.float() * s1[big.seg_d]) / 2.0)
    sn0, sn1 = _np(s0), _np(s1)
    assert np.isfinite(sn0).all() and (sn0[np.asarray(big.sizes) > 1] > 0).all()   # (one element: std 0, scalar 0)
    for s in big.spot:
        lo, hi = int(big.off[s]), int(big.off[s + 1])
        e0 = O.terngrad_decode(_np(c0[lo:hi]), sn0[s:s + 1])
        e1 = O.terngrad_decode(_np(c1[lo:hi]), sn1[s:s + 1])
        assert same_bits(_np(dec[lo:hi]), e0), s
        assert same_bits(_np(dec2[lo:hi]), (O.python_sum([e0, e1]) / F32(2)).astype(F32)), s


def test_general_decoder_second_round():
    """qsgd_decode_kernel past 4096 workgroups of one kDecRound round each: n = 4096 * 4096 + 12,345,
    bucket 100 over eight segments (int8) and the one-bucket global flavour (fp16), on random codes
    and norms: the whole array against the formula on the device, three slices against the oracle."""
    edge = 4096 * 4096
    n = edge + 12345
    assert -(-n // 4096) > 4096   # (kDecRound = 4096 elements, grid cap 4096)
    sizes = [4099, 1, 37, edge + 50 - 4137, 3, 12161, 129, 2]
    assert sum(sizes) == n
    g = torch.Generator(device=DEV)
    g.manual_seed(99)
    off = np.concatenate([[0], np.cumsum(sizes)])
    sub = np.concatenate([[0], np.cumsum([-(-s // 100) for s in sizes])])
    windows = [(0, 8192), (edge - 4096, edge + 4096), (n - 8192, n)]
    # bucket 100, q = 127
    codes = torch.randint(-127, 128, (n,), generator=g, device=DEV, dtype=torch.int8)
    norms = torch.rand(int(sub[-1]), generator=g, device=DEV) * 0.1 + 0.01
    out = ops.qsgd_decompress(codes, norms, 127, 100, n, sizes=sizes)
    seg_d = torch.repeat_interleave(torch.arange(len(sizes), device=DEV), torch.tensor(sizes, device=DEV))
    off_d, sub_d = torch.from_numpy(off).to(DEV), torch.from_numpy(sub).to(DEV)
    bidx = sub_d[seg_d] + (torch.arange(n, device=DEV) - off_d[seg_d]) // 100
    scale = _t((_np(norms) / F32(127)).astype(F32))
    assert dev_same(out, scale[bidx] * codes.float())
    del bidx, seg_d
    nn = _np(norms)
    for a, b in windows:
        for s in range(len(sizes)):   # the window's part of every segment, from a bucket boundary
            lo = max(a, int(off[s]))
            hi = min(b, int(off[s + 1]))
            if lo >= hi:
                continue
            lo -= (lo - int(off[s])) % 100
            b0 = int(sub[s]) + (lo - int(off[s])) // 100
            exp = O.qsgd_decode(_np(codes[lo:hi]), nn[b0:b0 + -(-(hi - lo) // 100)], 127, 100, hi - lo)
            assert same_bits(_np(out[lo:hi]), exp), (a, s)
    # one bucket of n, q = 255
    codes = torch.randint(-255, 256, (n,), generator=g, device=DEV, dtype=torch.int16).to(torch.float16)
    norm = torch.rand(1, generator=g, device=DEV) + 0.5
    out = ops.qsgd_global_decompress(codes, norm, 255, n)
    assert dev_same(out, _t((_np(norm) / F32(255)).astype(F32)) * codes.float())
    for a, b in windows:
        assert same_bits(_np(out[a:b]), O.qsgd_global_decode(_np(codes[a:b]), _np(norm), 255, b - a)), a


# ================================================================================================
# Part C: magnitude edges of the pipelined encoder's int8 shortcut
EDGE_K = 64
EDGE_SEED = 1163   # its draws have u < 2^-17 in three different buckets of the 64 (asserted below)


def _single_level(m, q):
    """level of the one non-zero element m of a bucket: norm = sqrt_f32(f32(m^2)), (1 / norm * q) |m|."""
    m = F32(m)
    with np.errstate(all="ignore"):
        norm = np.sqrt(F32(np.float64(m) * np.float64(m)), dtype=F32)
        return F32(F32(F32(1) / norm) * F32(q)) * abs(m)


def edge_buckets(q):
    """64 whole buckets, one case each: (x, u, names, round_up positions)."""
    n = 128 * EDGE_K
    u = qsgd_bucket128_uniforms(EDGE_SEED, [n])
    rng = np.random.default_rng(64)
    x = (rng.standard_normal((EDGE_K, 128)) * 0.01).astype(F32)   # unnamed buckets: ordinary data
    names = ["N(0, 0.01^2)"] * EDGE_K
    # a level a hair above q rounds up only under a tiny u: put those elements where the draws are tiny
    hits = {}
    for p in np.flatnonzero(u < F32(2.0 ** -17)):
        hits.setdefault(int(p) // 128, int(p))
    assert len(hits) >= 2, "EDGE_SEED no longer gives tiny draws in two buckets"
    m_up = F32(0.01)
    while not _single_level(m_up, q) > q:
        m_up = np.nextafter(m_up, F32(1))
    for i, (b, p) in enumerate(sorted(hits.items())):
        assert u[p] < _single_level(m_up, q) - F32(q)
        x[b] = 0.0
        x[b, p % 128] = m_up if i % 2 == 0 else -m_up
        names[b] = "one element, level above q, tiny u"
    free = iter(b for b in range(EDGE_K) if b not in hits)
    nrm = lambda s: (rng.standard_normal(128) * s).astype(F32)   # noqa: E731
    cases = [("N(0, 1e-19^2)", nrm(1e-19)), ("N(0, 1e-21^2)", nrm(1e-21)), ("N(0, 1e-37^2)", nrm(1e-37)),
             ("N(0, 1e-39^2)", nrm(1e-39)), ("all 3e19", np.full(128, 3e19, F32)),
             ("all -1e30", np.full(128, -1e30, F32)), ("+-3e19", np.where(np.arange(128) % 2, 3e19, -3e19).astype(F32)),
             ("all 0.01", np.full(128, 0.01, F32)), ("all -3", np.full(128, -3.0, F32)),
             ("all -0.0", np.full(128, -0.0, F32)), ("all +0.0", np.zeros(128, F32))]
    sub = 2.0 ** -149   # the smallest f32 subnormal: m^2 rounds to 2 sub / 1 sub, the norm falls short of m
    singles = [float(m_up), 0.01, 1.0, 3e-10, 1e10, 1e-30, 1e-40, 1.8e19, 3e19, np.sqrt(2.45 * sub),
               np.sqrt(1.45 * sub)]
    for i, m in enumerate(singles):
        for sg in (1.0, -1.0):
            v = np.zeros(128, F32)
            v[(7 * i + 3 + (sg < 0)) % 128] = F32(sg * m)
            cases.append(("one element %+.9g" % (sg * m), v))
    for name, v in cases:
        b = next(free)
        x[b], names[b] = v, name
    return x.reshape(-1), u, names, sorted(hits.values())


@pytest.mark.parametrize("q", [127, 255])
def test_pipelined_encoder_magnitude_edges(q):
    """qsgd_encode128_pipe_kernel, variant 0, its own draws: codes bit for bit the oracle's given the
    device norms at every magnitude edge (rows whose scale or norm is not finite take qsgd_code), and
    the norms within 1 ulp of the kernel's definition, sqrt_f32 of the f64 sum of exact squares rounded
    to f32.  (Not O.qsgd_norms: the reference squares in f32, and those squares underflow or overflow
    on their own here.  Printed, not asserted: the buckets whose codes differ from the ones the
    reference's f32 norms give; DESIGN.md's test table records them.)"""
    x, u, names, ups = edge_buckets(q)
    codes, norms = ops.qsgd_compress(_t(x), q, 128, seed=EDGE_SEED)
    cn, nn = _np(codes), _np(norms)
    with np.errstate(over="ignore"):
        ssq = (x.astype(np.float64).reshape(EDGE_K, 128) ** 2).sum(axis=1).astype(F32)
        ref_n = np.sqrt(ssq, dtype=F32)
    assert norms_close(nn, ref_n, 1), [(names[b], nn[b], ref_n[b]) for b in np.flatnonzero(nn != ref_n)]
    exp, _ = O.qsgd_compress(x, u, q, 128, norms=nn)
    bad = np.flatnonzero(cn.view(np.uint8 if q < 128 else np.uint16) != exp.view(np.uint8 if q < 128 else np.uint16))
    assert bad.size == 0, sorted({names[b] for b in bad // 128})
    # the cases are what they claim: a level at q rounded up (128 wraps to -128 in int8), norms that
    # overflowed, and scales that did
    for p in ups:
        assert abs(float(exp[p])) == (128 if q < 128 else q + 1), (p, exp[p])
    assert np.isinf(nn[names.index("all 3e19")]) and np.isinf(nn[names.index("all -1e30")])
    assert nn[names.index("N(0, 1e-39^2)")] == 0 and 0 < nn[names.index("N(0, 1e-21^2)")] < 1e-19
    with np.errstate(all="ignore"):
        assert np.isinf(F32(1) / nn[names.index("one element +1e-40")] * F32(q))
    ref, _ = O.qsgd_compress(x, u, q, 128)
    differ = sorted({names[b] for b in np.flatnonzero(ref != exp) // 128})
    print("q=%d: codes differ from the f32-reduction reference's in: %s" % (q, differ or "no bucket"))
