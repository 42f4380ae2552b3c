"""numpy restatement of grace_amd's own device generator (grace_amd/csrc/common.h: mix64, fmix32,
rand32, uniform01x4) -- test infrastructure, not the reference's algorithm (the reference draws from
torch's generators; rng="torch_cpu" reproduces those).  It lets the device-generator fast paths be
checked bit for bit: the uniforms a kernel draws on its own equal the ones restated here, so
``compress(x, seed=s)`` must equal ``compress(x, u=quad_uniforms(...))`` exactly.  Also the
standard normal stream of ops.normal (normal_stream, Box-Muller in float64), the f32 operation
chain of the PowerSGD outer product (outer_f32) and DGC's sample indices (dgc_sample_index)."""
import numpy as np

M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _fmix32(h):
    h = h.astype(np.uint64)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h


def _to_u01(h):
    return ((h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def quad_uniforms(seed, quad_start, lane):
    """uniform01x4(seed, quad_start)[lane] for element indices below 2^32 (rand32's high-word term
    is zero there)."""
    k = mix64(int(seed) & M64)
    klo, khi = np.uint64(k & 0xFFFFFFFF), np.uint64(k >> 32)
    e = np.asarray(quad_start, dtype=np.uint64)
    h = _fmix32((((e * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) ^ klo) + khi & np.uint64(0xFFFFFFFF))
    lane = np.asarray(lane)
    out = _to_u01(h)
    h = np.where(h == 0, np.uint64(0x9E3779B9), h)
    for j in range(1, 4):
        h ^= (h << np.uint64(13)) & np.uint64(0xFFFFFFFF)
        h ^= h >> np.uint64(17)
        h ^= (h << np.uint64(5)) & np.uint64(0xFFFFFFFF)
        out = np.where(lane == j, _to_u01(h), out)
    return out


def rand32(seed, i):
    """rand32(seed, i) of common.h on an array of element indices (any below 2^64), as uint64 words
    below 2^32."""
    m32 = np.uint64(0xFFFFFFFF)
    k = mix64(int(seed) & M64)
    i = np.asarray(i, dtype=np.uint64)
    h = ((i & m32) * np.uint64(0x9E3779B1)) ^ np.uint64(k & 0xFFFFFFFF) ^ ((i >> np.uint64(32)) * np.uint64(0x7FEB352D))
    return _fmix32(((h & m32) + np.uint64(k >> 32)) & m32)


def dgc_sample_index(seed, j, n):
    """dgc.hip's dgc_sample_index: the device generator's j-th DGC sample index into n elements,
    the high 64 bits of (rand32(seed, j) << 32 | rand32(seed ^ 0xD6E8FEB86659FD93, j)) * n.  int64
    array shaped like j."""
    n = int(n)
    hi = rand32(seed, j)
    lo = rand32((int(seed) & M64) ^ 0xD6E8FEB86659FD93, j)
    if n < (1 << 32):
        # (hi 2^32 + lo) n >> 64 in 64-bit words: hi n < 2^64, and the nested floors are exact
        return ((hi * np.uint64(n) + ((lo * np.uint64(n)) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)
    h = hi.astype(object) * (1 << 32) + lo.astype(object)
    return np.asarray((h * n) // (1 << 64), dtype=object).astype(np.int64)


def _mix64_np(z):
    """mix64 on a uint64 array (the arithmetic wraps modulo 2^64 as on the device)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def normal_stream(seed, n, with_rad=False):
    """The first n standard normal draws of ops.normal(..., seed) (grace_amd/csrc/powersgd.hip
    normal_pair): the hash and the two uniforms exactly as the device computes them (integer mix,
    f32 conversions and f32 multiplies), then Box-Muller in float64 where the device uses its f32
    hardware log2 / sqrt / sin / cos.  Element e is component e & 1 of pair e >> 1.  with_rad: also
    the radius sqrt(-2 ln u1) of every element's pair (the scale of the device's rounding error)."""
    npair = (int(n) + 1) // 2
    pair = np.arange(npair, dtype=np.uint64)
    h = _mix64_np(np.uint64(int(seed) & M64) ^ _mix64_np(pair * np.uint64(2) + np.uint64(1)))
    # 1.0f / 16777217.0f: the f32 literal 16777217 is 2^24 (ties to even), so u1 lies in (0, 1]
    k1 = np.float32(1.0) / np.float32(16777217.0)
    u1 = ((h >> np.uint64(40)).astype(np.float32) + np.float32(1.0)) * k1
    u2 = (h & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    ang = 2.0 * np.pi * u2.astype(np.float64)
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).reshape(-1)[:n]
    if with_rad:
        return z, np.repeat(rad, 2)[:n]
    return z


def normal_moment_bounds(z):
    """The three 5-sigma moment checks of a standard normal sample laid out as Box-Muller pairs:
    (|mean|, |var - 1|, |corr(z0, z1)|) each divided by its bound -- all must be below 1."""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    mean, var = z.mean(), z.var()
    z0, z1 = z[0:n - (n & 1):2], z[1::2]
    corr = np.mean((z0 - z0.mean()) * (z1 - z1.mean())) / (z0.std() * z1.std())
    return abs(mean) / (5 / np.sqrt(n)), abs(var - 1) / (5 * np.sqrt(2 / n)), abs(corr) / (5 / np.sqrt(n / 2))


NORMAL_SEEDS = (4242, 7)                       # the seeds the normal-stream tests draw with (CPU and GPU)
NORMAL_ZMAX = np.sqrt(2 * 24 * np.log(2))      # u1 >= 2^-24


def outer_f32(P, Q):
    """P Q^T in the exact f32 operation chain of psgd_outer_kernel / psgd_outer4_kernel (the library
    is built without fused multiply-add): o = 0, then o = f32(o + f32(p[c] * q[c])) for c = 0..r-1."""
    P = np.asarray(P, dtype=np.float32)
    Q = np.asarray(Q, dtype=np.float32)
    o = np.zeros((P.shape[0], Q.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for c in range(P.shape[1]):
            o = o + P[:, c:c + 1] * Q[None, :, c]
    assert o.dtype == np.float32
    return o


def qsgd_bucket128_uniforms(seed, sizes, segs=None):
    """The uniform each element of the segmented QSGD(bucket 128) encoders draws: the quad of element
    i starts at its bucket's base + 4 * ((i - base) // 4) (grace_amd/csrc/quant.hip).
    segs=(lo, hi): only the draws of segments lo .. hi - 1 (the elements sum(sizes[:lo]) ..
    sum(sizes[:hi]) - 1), with index arrays over those elements alone."""
    sizes = np.asarray(sizes, dtype=np.int64)
    lo, hi = (0, len(sizes)) if segs is None else segs
    part = sizes[lo:hi]
    first = int(sizes[:lo].sum())
    starts = first + np.concatenate([[0], np.cumsum(part)[:-1]]).astype(np.int64)
    seg = np.repeat(np.arange(len(part)), part)
    i = first + np.arange(int(part.sum()), dtype=np.int64)
    rel = i - starts[seg]
    base = starts[seg] + (rel // 128) * 128
    qs = base + ((i - base) // 4) * 4
    return quad_uniforms(seed, qs, i - qs)
