"""The device sampler of the GLM (sampler="device") as a specification: which standard normal the draw for (seed, step, weight
sample kl, feature f) is -- in plain integers and in NumPy, written from the formula, importing nothing of the package -- with
the case tables and the "identity" set-ups that make the device's draws observable (pure numpy; shared by
tests/test_sampler_cases_host.py and tests/test_gpu_sampler_exact.py).

    splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
                   x = (x ^ x >> 27) * 0x94D049BB133111EB; return x ^ x >> 31                (mod 2^64)
    key = splitmix64(seed ^ (step * 0xD1B54A32D192ED03))
    h   = splitmix64(key ^ ctr),  ctr = kl F + f,  kl = k L + l       (F the feature count, not a padded row length)
    u1  = ((h >> 40) + 1) / 2^24 in (0, 1];   u2 = ((h >> 8) & 0xFFFFFF) / 2^24 in [0, 1)
    e   = sqrt(-2 ln u1) cos(2 pi u2)

The device evaluates the last line in float32 (__logf, the hardware cosine on revolutions); the model in float64 from the
same two integers.  The generator is rr_svi_stepkey / rr_svi_draw (rr_svi_common.h); the kernels that call it: rr_glm_draw_kernel
(rr_elbo.hip: rr_featmat_glm_step_sampled and the resident step rr_glm_sgd_step), svi_draws (rr_svi.hip: the fused loop's step
0, its prefetch of step t + 1, and the random starts) and sw_draws (rr_svi_wide.hip).  The fused loop's launch step t uses step = key0 + t, candidate c of its starts step = key0 + c.

The identity set-up: a linear child without the column of ones on X = I_F, Gaussian likelihood with variance 1, y = 0, m = 0,
C a power of four.  The latent value of row r under weight sample kl is then the weight itself, w = sqrt(C) e, exactly -- the
division by K L (a power of two) before the float32 product with a 1 and the multiplication after it round nothing -- df = -w
and Edws[kl][f] = -sqrt(C[f][k]) e[kl][f].  With L = 1:  Edm[f][k] = -sqrt(C) e,  EdC[f][k] = Edws e / sqrt(C) = -e^2,  so that
EdC C == -Edm^2 bit for bit in float64 (a product of two float32 values is exact there): the premise of exact recovery, checked
without the model."""
import numpy as np

MASK64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
MUL1 = 0xBF58476D1CE4E5B9
MUL2 = 0x94D049BB133111EB
STEP_MUL = 0xD1B54A32D192ED03
E_MAX = float(np.sqrt(48 * np.log(2.0)))   # u1 = 2^-24, u2 = 0: 5.768


# ---- plain integers --------------------------------------------------------------------------------------------------------
def splitmix64_int(x):
    x = (x + GAMMA) & MASK64
    x = ((x ^ (x >> 30)) * MUL1) & MASK64
    x = ((x ^ (x >> 27)) * MUL2) & MASK64
    return x ^ (x >> 31)


def key_int(seed, step):
    return splitmix64_int((seed ^ ((step * STEP_MUL) & MASK64)) & MASK64)


def hash_bits_int(h):
    """(u1 2^24, u2 2^24) of a hash: bits 40-63 (+ 1) and bits 8-31"""
    return (h >> 40) + 1, (h >> 8) & 0xFFFFFF


def model_bits_int(seed, step, ctr):
    return hash_bits_int(splitmix64_int(key_int(seed, step) ^ ctr))


# ---- NumPy, vectorised -----------------------------------------------------------------------------------------------------
def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def splitmix64(x):
    with np.errstate(over="ignore"):
        x = _u64(x) + np.uint64(GAMMA)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(MUL1)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(MUL2)
    return x ^ (x >> np.uint64(31))


def key(seed, step):
    with np.errstate(over="ignore"):
        return splitmix64(_u64(seed) ^ (_u64(step) * np.uint64(STEP_MUL)))


def hash_bits(h):
    h = _u64(h)
    return (h >> np.uint64(40)).astype(np.int64) + 1, ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64)


def model_bits(seed, step, ctr):
    """(u1 2^24, u2 2^24) as int64 arrays; seed, step, ctr broadcast against each other."""
    return hash_bits(splitmix64(key(seed, step) ^ _u64(ctr)))


def normal_of_bits(a, b):
    """e = sqrt(-2 ln u1) cos(2 pi u2) in float64 from the two 24-bit integers"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.sqrt(-2.0 * np.log(a / 16777216.0)) * np.cos(2.0 * np.pi * (b / 16777216.0))


def model_stream(seed, step, n):
    """The draws of counters 0 .. n - 1, float64 (n,)"""
    return normal_of_bits(*model_bits(seed, step, np.arange(n, dtype=np.uint64)))


def model_draws(seed, step, K, L, F):
    """float64 (K L, F): row kl = k L + l, column f, counter kl F + f"""
    return model_stream(seed, step, K * L * F).reshape(K * L, F)


# ---- case tables -----------------------------------------------------------------------------------------------------------
# host: (seed, step) of the distribution checks; the conditions at 2^20 draws (about four standard errors)
DIST_KEYS = [(0, 0), (1, 0), (123456789, 7), (2 ** 31 - 2, 1000)]
DIST_BOUNDS = {"mean": 4e-3, "var": 6e-3, "skew": 1e-2, "kurt": 2e-2, "ks": 2e-3, "corr": 4e-3}
DIST_LAGS = (1, 37)
# known answers
SPLITMIX_STATE = 1234567
SPLITMIX_OUT = [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]
KNOWN_KEY = (11, 3)
KNOWN_U1 = [10895965, 6119926, 9308294, 3831685]
KNOWN_U2 = [10498157, 5427366, 15532406, 9728730]

# device.  A: F = 37 (one pad block) and 300 (crosses a 256-column pad block: the row length in HBM is 512), K L = 64
STEP_F = (37, 300)
STEP_KL = 64
STEP_SEEDS = (11, 2 ** 31 + 12345)       # the second does not fit a signed 32-bit integer
STEP_STEPS = (0, 7)
STEP_FACTORINGS = ((8, 8), (4, 16))      # (K, L) with K L = 64
STEP_WIDE = (8, 64)                      # K L = 512: widens the step scratch before the K L = 64 case runs again
# B, C, D: the loops
LOOP_SEED = 11
LOOP_K = 4
LOOP_KEYS = (5, 6, 7)
SVI_F = (38, 37)                         # the fused kernel's row length in LDS is F | 1: 39 for F = 38
SVI_KL = (2, 8)                          # (K, L) of the sample-averaged case and of the starts
SVI_M = 19                               # rows of I_F per fused step: the kernel's gather takes M F <= 1024 entries


def svi_rows(F, t):
    """The rows of I_F fused step (or candidate) t works on: 0-18, 11-29, 22-40 mod F -- together every row"""
    return (11 * t + np.arange(SVI_M)) % F
STARTS_KEY0 = 9
B_CAP = 1e-5                             # the bound on |e_device - e_model| may not exceed this


# ---- the identity set-up ---------------------------------------------------------------------------------------------------
def power_of_four_C(F, K):
    """C[f][k] = 4^-(k mod 3): sqrt(C) is a power of two that changes with the component"""
    return np.tile(4.0 ** -(np.arange(K) % 3), (F, 1))


def identity_step(F, K):
    """(X, y, m, C) of one rr_featmat_glm_step_sampled call"""
    return np.eye(F), np.zeros(F), np.zeros((F, K)), power_of_four_C(F, K)


def draws_from_step(Edm, EdC, C):
    """e (K, F) from the (F, K) outputs of an L = 1 identity step, after the model-free check of the premise."""
    Edm, EdC, C = np.asarray(Edm), np.asarray(EdC), np.asarray(C)
    assert np.array_equal(EdC * C, -(Edm * Edm)), "EdC C != -Edm^2: the step rounded something, no exact recovery"
    return (-Edm / np.sqrt(C)).T.copy()


def reduced_from_draws(e, K, L, C):
    """(Edm, EdC) (F, K) of an identity step with L samples per component, from the draws e (K L, F): the sums over l in the
    kernel's order (rr_glm_reduce_kernel: l ascending, in float64)."""
    F = e.shape[1]
    e = e.reshape(K, L, F)
    s = np.sqrt(C).T                          # (K, F)
    a, b = np.zeros((K, F)), np.zeros((K, F))
    for l in range(L):
        ed = -s * e[:, l]                     # Edws, a float32 value
        a = a + ed
        b = b + ed * e[:, l]
    return (a / L).T, (b / (L * s)).T


def loop_z0(F, K, C=1.0, reg=1.0, var=1.0):
    """[m = 0 | C | reg | var] of a loop with one linear child and a Gaussian likelihood"""
    return np.concatenate([np.zeros(F * K), np.broadcast_to(np.asarray(C, dtype=float), (F, K)).ravel(), [reg, var]])


def starts_C(F, K):
    """C[f][k] = (1 + (f + 38 k) / 64)^2: a weight of its own on every coordinate"""
    f, k = np.meshgrid(np.arange(F), np.arange(K), indexing="ij")
    return (1.0 + (f + 38 * k) / 64.0) ** 2


# ---- statistics ------------------------------------------------------------------------------------------------------------
def moments(x):
    """(mean, var - 1, skewness, excess kurtosis)"""
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean()
    d = x - mu
    v = (d * d).mean()
    return mu, v - 1.0, (d ** 3).mean() / v ** 1.5, (d ** 4).mean() / v ** 2 - 3.0


def ks_normal(x):
    """Kolmogorov-Smirnov distance to N(0, 1)"""
    from scipy.special import ndtr
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    cdf = ndtr(x)
    i = np.arange(1, n + 1)
    return float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max()))


def corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
