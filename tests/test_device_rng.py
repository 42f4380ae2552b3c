"""CPU checks of the numpy restatement of the device generator (tests/device_rng.py)."""
import numpy as np
import pytest

from tests.device_rng import (NORMAL_SEEDS, NORMAL_ZMAX, _mix64_np, dgc_sample_index, mix64, normal_moment_bounds,
                              normal_stream, outer_f32, qsgd_bucket128_uniforms, quad_uniforms, rand32)


def test_mix64_is_splitmix64():
    # splitmix64's first output from state 0 (the published known answer)
    assert mix64(0) == 0xE220A8397B1DCDAF


def test_mix64_array_form_matches_scalar():
    z = [0, 1, 12345, (1 << 64) - 1, 0x9E3779B97F4A7C15]
    assert [int(v) for v in _mix64_np(np.array(z, dtype=np.uint64))] == [mix64(v) for v in z]


@pytest.mark.parametrize("seed", NORMAL_SEEDS)
def test_normal_stream_is_standard_normal(seed):
    n = 1 << 22
    z = normal_stream(seed, n)
    assert z.dtype == np.float64 and z.shape == (n,)
    assert np.isfinite(z).all() and np.abs(z).max() <= NORMAL_ZMAX * (1 + 1e-6)
    assert max(normal_moment_bounds(z)) < 1, normal_moment_bounds(z)
    # a prefix of the stream is the stream (element e = component e & 1 of pair e >> 1)
    assert np.array_equal(normal_stream(seed, 7), z[:7])
    z2, rad = normal_stream(seed, 9, with_rad=True)
    assert np.allclose(np.hypot(z2[0:8:2], z2[1:8:2]), rad[0:8:2], rtol=1e-12)
    assert np.isclose(rad[8], np.hypot(z[8], z[9]), rtol=1e-12)


def test_outer_f32_vs_f64():
    rng = np.random.default_rng(1)
    for n, m, r in ((37, 1029, 1), (37, 1029, 16), (5, 64, 4), (1, 4, 7)):
        P = rng.standard_normal((n, r)).astype(np.float32)
        Q = rng.standard_normal((m, r)).astype(np.float32)
        o = outer_f32(P, Q)
        assert o.dtype == np.float32 and o.shape == (n, m)
        P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
        assert np.all(np.abs(o - P64 @ Q64.T) <= r * 2.0 ** -24 * (np.abs(P64) @ np.abs(Q64).T))
    # the chain starts from +0: (-0) * q gives -0, and 0 + (-0) = +0
    o = outer_f32(np.array([[-0.0]], dtype=np.float32), np.array([[3.0]], dtype=np.float32))
    assert not np.signbit(o[0, 0])


DGC_SEEDS = (0, 123, 2 ** 63 + 5)


def test_rand32_matches_quad_uniforms_hash():
    # uniform01x4's first lane is rand32's top 24 bits
    e = np.arange(0, 4096, 4)
    u = (rand32(7, e) >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    assert np.array_equal(u, quad_uniforms(7, e, np.zeros(e.size, dtype=np.int64)))


@pytest.mark.parametrize("seed", DGC_SEEDS)
def test_dgc_sample_index_range_and_uniformity(seed):
    for n in (1, 99, 100003, 1 << 20, 6553600):
        ns = max(1, int(n * 0.01))
        i = dgc_sample_index(seed, np.arange(ns), n)
        assert i.dtype == np.int64 and i.shape == (ns,)
        assert i.min() >= 0 and i.max() < n, (seed, n)
    # the 64-bit word form equals the 128-bit product in Python integers, at n past 2^32 too
    for n in (99, 6553600, (1 << 32) - 1, (1 << 40) + 7):
        j = np.array([0, 1, 77, 65535, (1 << 33) + 3], dtype=np.uint64)
        hi, lo = rand32(seed, j), rand32((seed & ((1 << 64) - 1)) ^ 0xD6E8FEB86659FD93, j)
        want = [(((int(h) << 32) | int(l)) * n) >> 64 for h, l in zip(hi, lo)]
        assert dgc_sample_index(seed, j, n).tolist() == want
    # chi-square over 64 equal bins of [0, n): 63 degrees of freedom, mean 63, sd sqrt(126) = 11.2;
    # the bound is the mean plus six standard deviations
    ns, n, bins = 65536, 6553600, 64
    i = dgc_sample_index(seed, np.arange(ns), n)
    obs = np.bincount(i // (n // bins), minlength=bins).astype(np.float64)
    assert obs.size == bins
    chi2 = float(((obs - ns / bins) ** 2 / (ns / bins)).sum())
    print(f"seed {seed}: chi-square {chi2:.1f}")
    assert chi2 <= 130, (seed, chi2)


def test_quad_uniforms_range_and_quads():
    u = quad_uniforms(7, np.repeat(np.arange(0, 4096, 4), 4), np.tile(np.arange(4), 1024))
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert abs(float(u.mean()) - 0.5) < 0.02
    # segments restart the bucket grid: an unaligned segment's quads start at its own bucket base
    v = qsgd_bucket128_uniforms(7, [5, 130])
    assert np.array_equal(v[5:9], quad_uniforms(7, [5] * 4, np.arange(4)))
    assert np.array_equal(v[133:135], quad_uniforms(7, [133] * 2, np.arange(2)))


def test_qsgd_bucket128_uniforms_segment_range():
    """segs=(lo, hi) gives exactly the full function's draws of those segments: aligned and
    unaligned starts, partial buckets, one-element segments, the first, the last and no segment."""
    sizes = [128 * 3, 5, 3, 128 * 2, 130, 1, 15, 256, 7]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    full = qsgd_bucket128_uniforms(99, sizes)
    assert full.size == offs[-1]
    for lo, hi in [(0, len(sizes)), (0, 1), (1, 4), (2, 3), (4, 9), (8, 9), (5, 5)]:
        part = qsgd_bucket128_uniforms(99, sizes, segs=(lo, hi))
        assert part.dtype == np.float32
        assert np.array_equal(part, full[offs[lo]:offs[hi]]), (lo, hi)
