"""The specification of the device sampler (tests/sampler_cases.py) on the host: its two statements -- Python integers with
masks, NumPy uint64 -- against known answers and against each other, the structure of the generator (distinct step keys, u1
never 0, |e| bounded, disjoint bit fields) and the distribution of the float64 model.  What the GPU computes is held to this
model by tests/test_gpu_sampler_exact.py; here the model itself is shown to be the standard normal it claims to be, at
conditions of about four standard errors of 2^20 draws (2^16: the same, times 4)."""
import numpy as np
import pytest

import sampler_cases as sc


# ---- known answers -----------------------------------------------------------------------------------------------------------
def test_splitmix64_published_vectors():
    """The generator's stream from state 1234567 (state += gamma; output = mix(state)): splitmix64(x) here is mix(x + gamma)."""
    got = [sc.splitmix64_int((sc.SPLITMIX_STATE + i * sc.GAMMA) & sc.MASK64) for i in range(5)]
    assert got == sc.SPLITMIX_OUT
    state = np.array([(sc.SPLITMIX_STATE + i * sc.GAMMA) & sc.MASK64 for i in range(5)], dtype=np.uint64)
    assert sc.splitmix64(state).tolist() == sc.SPLITMIX_OUT


def test_known_bits_of_seed_11_step_3():
    seed, step = sc.KNOWN_KEY
    got = [sc.model_bits_int(seed, step, c) for c in range(4)]
    assert [g[0] for g in got] == sc.KNOWN_U1 and [g[1] for g in got] == sc.KNOWN_U2
    a, b = sc.model_bits(seed, step, np.arange(4))
    assert a.tolist() == sc.KNOWN_U1 and b.tolist() == sc.KNOWN_U2


def test_the_two_statements_agree_on_random_arguments():
    """10^5 random (seed, step, ctr) over the whole 64-bit range, the small values a fit uses, and the corners."""
    rs = np.random.RandomState(5)

    def rand64(n):
        return (rs.randint(0, 2 ** 32, size=n).astype(np.uint64) << np.uint64(32)) | rs.randint(0, 2 ** 32, size=n).astype(np.uint64)
    n = 50000
    seed = np.concatenate([rand64(n), rs.randint(0, 2 ** 31 - 1, size=n).astype(np.uint64)])
    step = np.concatenate([rand64(n), rs.randint(0, 100000, size=n).astype(np.uint64)])
    ctr = np.concatenate([rand64(n), rs.randint(0, 2 ** 26, size=n).astype(np.uint64)])
    corner = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 63, sc.MASK64], dtype=np.uint64)
    cs, ct, cc = (v.ravel() for v in np.meshgrid(corner, corner, corner))
    seed, step, ctr = np.concatenate([seed, cs]), np.concatenate([step, ct]), np.concatenate([ctr, cc])
    assert seed.size >= 100000
    a, b = sc.model_bits(seed, step, ctr)
    want = [sc.model_bits_int(int(s), int(t), int(c)) for s, t, c in zip(seed.tolist(), step.tolist(), ctr.tolist())]
    assert a.tolist() == [w[0] for w in want]
    assert b.tolist() == [w[1] for w in want]
    assert sc.key(seed, step).tolist() == [sc.key_int(int(s), int(t)) for s, t in zip(seed.tolist(), step.tolist())]


# ---- structure -----------------------------------------------------------------------------------------------------------------
def test_step_keys_are_distinct():
    s, t = np.meshgrid(np.arange(64), np.arange(64))
    keys = sc.key(s.ravel(), t.ravel())
    assert np.unique(keys).size == 4096
    assert len({sc.key_int(a, b) for a in range(64) for b in range(64)}) == 4096


def test_bit_fields_are_disjoint_and_bounded():
    """u1 2^24 in [1, 2^24] (never 0: the logarithm is finite), u2 2^24 in [0, 2^24); a bit of the hash moves at most one of the
    two: bits 40-63 u1, bits 8-31 u2, bits 0-7 and 32-39 neither."""
    assert sc.hash_bits_int(0) == (1, 0) and sc.hash_bits_int(sc.MASK64) == (1 << 24, (1 << 24) - 1)
    rs = np.random.RandomState(1)
    for h in [0, sc.MASK64] + [int(rs.randint(0, 2 ** 32)) << 32 | int(rs.randint(0, 2 ** 32)) for _ in range(50)]:
        a, b = sc.hash_bits_int(h)
        assert 1 <= a <= 1 << 24 and 0 <= b < 1 << 24
        for bit in range(64):
            a2, b2 = sc.hash_bits_int(h ^ (1 << bit))
            assert (a2 != a) == (bit >= 40), bit
            assert (b2 != b) == (8 <= bit < 32), bit
        av, bv = sc.hash_bits(np.array([h], dtype=np.uint64))
        assert (int(av[0]), int(bv[0])) == (a, b)


def test_draws_are_finite_and_bounded():
    """|e| <= sqrt(48 ln 2) = 5.77, reached at u1 = 2^-24, u2 = 0; u1 = 1 gives 0."""
    assert sc.E_MAX == pytest.approx(5.768, abs=1e-3)
    assert sc.normal_of_bits(1, 0) == pytest.approx(sc.E_MAX, rel=1e-15)
    assert sc.normal_of_bits(1, 1 << 23) == pytest.approx(-sc.E_MAX, rel=1e-15)
    assert sc.normal_of_bits(1 << 24, 12345) == 0.0
    for seed, step in sc.DIST_KEYS:
        a, b = sc.model_bits(seed, step, np.arange(1 << 20))
        assert a.min() >= 1 and a.max() <= 1 << 24 and b.min() >= 0 and b.max() < 1 << 24
        e = sc.normal_of_bits(a, b)
        assert np.all(np.isfinite(e)) and np.abs(e).max() <= sc.E_MAX


def test_model_draws_layout():
    """Row kl, column f is counter kl F + f -- with F the feature count -- and depends on K L only through kl."""
    e = sc.model_draws(11, 3, 2, 3, 5)
    assert e.shape == (6, 5) and e.dtype == np.float64
    flat = sc.normal_of_bits(*sc.model_bits(11, 3, np.arange(30)))
    assert np.array_equal(e.ravel(), flat)
    assert np.array_equal(sc.model_draws(11, 3, 3, 2, 5), e)
    assert np.array_equal(sc.model_draws(11, 3, 1, 2, 5), e[:2])
    assert e[0, 0] == sc.normal_of_bits(sc.KNOWN_U1[0], sc.KNOWN_U2[0])


# ---- distribution ----------------------------------------------------------------------------------------------------------
_STREAMS = {}


def _stream(seed, step):
    if (seed, step) not in _STREAMS:
        _STREAMS[(seed, step)] = sc.model_stream(seed, step, 1 << 20)
    return _STREAMS[(seed, step)]


@pytest.mark.parametrize("log2n,scale", [(20, 1.0), (16, 4.0)], ids=["2^20", "2^16"])
@pytest.mark.parametrize("seed,step", sc.DIST_KEYS)
def test_distribution_of_the_model(seed, step, log2n, scale):
    """Moments, Kolmogorov-Smirnov distance to N(0, 1), and correlations: at lags 1 and 37 within a stream, between steps s and
    s + 1 of one seed and between seeds s and s + 1 of one step.  2^16: the counters of the (K L, F) slabs a fit uses."""
    n = 1 << log2n
    x = _stream(seed, step)[:n]
    bnd = {k: v * scale for k, v in sc.DIST_BOUNDS.items()}
    mean, dvar, skew, kurt = sc.moments(x)
    got = {"mean": abs(mean), "var": abs(dvar), "skew": abs(skew), "kurt": abs(kurt), "ks": sc.ks_normal(x)}
    cs = [abs(sc.corr(x[:-lag], x[lag:])) for lag in sc.DIST_LAGS]
    cs.append(abs(sc.corr(x, sc.model_stream(seed, step + 1, n))))
    cs.append(abs(sc.corr(x, sc.model_stream(seed + 1, step, n))))
    got["corr"] = max(cs)
    print("MEASURED model distribution seed=%d step=%d n=2^%d: %s" % (
        seed, step, log2n, " ".join("%s=%.2e" % (k, got[k]) for k in sorted(got))))
    bad = {k: (got[k], bnd[k]) for k in got if not got[k] < bnd[k]}
    assert not bad, bad
