"""Every route of the device posterior (rr_posterior_dev, rr_variance_factor_dev; rr_posdef.hip) against exact references,
bit for bit: C, m, diag C and sum(G o C) with `==`, log|iC| to the rounding of its host sum.

The data.  The upper factor is built directly, U = D + N: D diagonal with powers of two in [1/4, 4] ([1/8, 8] up to 100
columns), N strictly upper triangular with entries in {+-1, +-2} and N[i, j] != 0 only where i < j and level(i) < level(j),
level(i) = (i - F) mod 3 -- three levels, the last column on the top one, so that a ragged last panel of a single column
is still coupled to every panel above it --, filled at density `density(F)` among those positions (1 up to 320 columns, 1/2
up to 1280, 1/4 above: as dense as the bounds below allow, so that C needs more than 24 bits at every size from 64 up).  A
path through N climbs the three levels, so with M = D^-1 N: M^3 = 0 and U^-1 = (I - M + M^2) D^-1, a short dyadic matrix.
The inputs are iC = U^T U, iL small positive integers, var = 1/2, G = (iC - diag(iL)) var and b integer in [-3, 3].
Then every number the device forms is a dyadic rational with few bits:

* every Schur complement is a partial sum of iC - sum u u^T (multiples of q_U^2, below 2 |U|^T |U|), the pivots are exactly
  d^2 = 4^k, -3 <= k <= 3, and rr_sqrt_and_rsqrt returns exactly d and 1 / d for them whatever the seed of v_rsq_f64
  (tests/test_host_logic.py::test_coupled_sqrt_and_rsqrt_is_exact_at_powers_of_four_for_any_seed);
* every diagonal block's inverse is a block of the same family: dyadic, below A = (I + |M| + |M|^2) |D^-1| entry by entry;
* the panel solves U_j,> = U_jj^-T S_j,> add multiples of q_Ui q_U^2 below A^T (|U|^T |U|); the substitution Y = U^-T adds
  multiples of q_U q_Ui below I + |N|^T A^T and scales them by U_jj^-T (multiples of q_Ui^2 q_U below A^T (I + |N|^T A^T));
  C = Y^T Y adds multiples of q_Ui^2 below A A^T; m = C b / var multiples of q_C below |C| |b| (1 / var = 2); sum(G o C)
  products that are exact (bit counts asserted) and multiples of one quantum, below sum |G| |C|.

`_check_exact` computes the quanta q from the data (the lowest set bit over a matrix) and asserts each bound over its quantum
below 2^53: every partial sum of every one of these sums, in ANY order, over any K-split, in an MFMA accumulator, an f64
atomic or a deterministic slab, is then a representable number and the result does not depend on the route.  It also
asserts that C needs more than 24 bits -- one float32 step anywhere would change it.  An ISOLATED index k (row and column k
of N zero) takes part in no sum with a second term; its d_k may be any power of two (2^-16 and 2^-17 around CHOLTHRESH =
1e-5; 2^-24 for the variance factor's fallback) and stays out of the quanta.  F is padded to 128-column panels with the
identity, which is a member of the family (d = 1, N = 0).

Sensitivity (`_check_sensitive`, on the CPU, once per size): for all panels p < a <= b the block product U[p,a]^T U[p,b] of
the trailing update is nonzero, and for all c <= p < a the substitution's U[p,a]^T Y[p,c]: a dropped tile or a dropped block
row of a K = 256 pair changes the result.  (Shown by x^T (U[p,a]^T U[p,b]) z != 0 for two integer vectors.)

The routes.  `gemm_kernel`, `pipeline_calls` and `predicted_launches` restate rr_launch_gemm_tn_f64's rule, the loops of
rr_posterior_dev and chol_upper_blocked, and launch_chol_diag; `test_cases_cover_every_route` asserts from them that the
sizes below and the switches reach every schedule branch and both kernels of every product that can take both;
tests/test_debug_builds.py::test_bounds_build_counts_the_posterior_kernel_each_route_takes holds the restated rules to the
launch counts of the bounds-checking build.  Switches read once per process run in a child process each (`guarded_child`
of test_gpu_gram_exact.py: none is started after one that failed or hung).
"""
import functools
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu

PB = 128
VAR = 0.5
DVALS = [0.25, 0.5, 1.0, 2.0, 4.0]
DVALS_SMALL = [0.125] + DVALS + [8.0]     # up to 100 columns: a wider diagonal, for C to need more than 24 bits there too


def density(F):
    return 1.0 if F <= 320 else 0.5 if F <= 1280 else 0.25


LIMIT = 2.0 ** 53
SENTINEL = 0x7FF8C0DEC0DEC0DE      # a quiet NaN's bits: never a result, and != itself as a number
CHOLTHRESH = 1e-5

CHOL_KERNELS = ["rr_chol_diag_kernel", "rr_chol_diag_pipe_kernel", "rr_chol_diag_mfma_kernel"]
KERNELS = CHOL_KERNELS + ["rr_gemm_tn_f64_k128_kernel", "rr_gemm_tn_f64_kernel", "rr_syrk_f64_kernel", "rr_syrk_f64_diag_kernel",
                          "rr_posterior_coop_kernel", "rr_posterior_rows_kernel", "rr_reverse_pad_kernel",
                          "rr_ul_factor_f32_kernel", "rr_c64_to_c32_kernel"]

# ---- the cases ----------------------------------------------------------------------------------------------------------
PIPELINE_F = [1, 5, 127, 128,                                   # nblk = 1: one stream
              129, 200, 256,                                    # nblk = 2: second stream, no look-ahead
              257, 300, 384, 512, 700, 1000, 1024, 1153, 1280,  # look-ahead on the third stream, no pairs
              4400]                                             # Fp = 4480: panels 0-1 and 2-3 are pairs, 31 unpaired ones follow
SMALL_F = [1, 5, 64, 100, 256, 300, 512, 1000, 1024]            # RR_POSDEF_SMALL=1: the cooperative kernel
REFUSAL_F = [100, 200, 700, 1153]
FACTOR_F = [1, 100, 128, 129, 300, 700, 1153]
CHILD_F = [128, 256, 384, 512, 640, 1153, 1280]                 # 1, 2, 3, 4, 5, 10 (ragged), 10 panels
# read once per process (static const in rr_posterior_dev, launch_chol_diag, rr_launch_gemm_tn_f64)
VARIANTS = [{"RR_POSDEF_OVERLAP": "0"}, {"RR_POSDEF_LOOKAHEAD": "0"}, {"RR_POSDEF_PAIR_MIN": "256"}, {"RR_POSDEF_PAIR_MIN": "512"},
            {"RR_POSDEF_PAIR": "0", "RR_POSDEF_PAIR_MIN": "256"}, {"RR_POSDEF_EARLY_CHECK": "1"}, {"RR_CHOL_DIAG": "0"},
            {"RR_CHOL_DIAG": "1"}, {"RR_GEMM64_K128": "0"},
            {"RR_GEMM64_K128": "0", "RR_POSDEF_PAIR_MIN": "256"}]   # (the pairs' one-tile products on the tile kernel: only so)
SWITCHES = sorted({k for v in VARIANTS for k in v} | {"RR_POSDEF_SMALL"})
# measured on an MI355X (docs/KERNELS.md): the default child takes 2.5 s, most of it the start of the process and the
# references; the limit leaves a busy machine a factor of 40, the census (bounds-checking build, 2.7 s) twice that
CHILD_TIMEOUT = 100


def variant_id(v):
    return ",".join("%s=%s" % kv for kv in sorted(v.items())) or "default"


# ---- the launch rules, restated -----------------------------------------------------------------------------------------
def gemm_kernel(K, M, N, upper_only, env):
    """rr_launch_gemm_tn_f64 (rr_rff.hip): the whole-K register kernel for one 128-row tile, the tile kernel otherwise."""
    no_k128 = env.get("RR_GEMM64_K128") is not None and int(env["RR_GEMM64_K128"]) == 0
    if not no_k128 and K == 128 and M == 128 and N % 32 == 0 and (upper_only == 0 or (upper_only == 1 and N == 128)):
        return "rr_gemm_tn_f64_k128_kernel"
    return "rr_gemm_tn_f64_kernel"


def schedule(F, env):
    """The switches of rr_posterior_dev's loop at F columns: (nblk, overlap, lookahead, pair_on, pair_min)."""
    nblk = (F + PB - 1) // PB
    off = lambda name: env.get(name) is not None and int(env[name]) == 0
    overlap = not off("RR_POSDEF_OVERLAP") and nblk > 1
    lookahead = overlap and not off("RR_POSDEF_LOOKAHEAD") and nblk > 2
    pair_on = lookahead and not off("RR_POSDEF_PAIR")
    pair_min = int(env["RR_POSDEF_PAIR_MIN"]) if env.get("RR_POSDEF_PAIR_MIN") else 4096
    return nblk, overlap, lookahead, pair_on, pair_min


def pipeline_calls(F, env):
    """[(branch, site, K, M, N, upper_only)] of every rr_launch_gemm_tn_f64 call of one rr_posterior_dev at F columns, in
    program order.  branch: 'one stream' | 'overlap' | 'lookahead' | 'first of a pair' | 'second of a pair' |
    'unpaired after pairs'; site: the call's place in the loop."""
    nblk, overlap, lookahead, pair_on, pair_min = schedule(F, env)
    Fp, out, paired = nblk * PB, [], False
    for j in range(nblk):
        rest, width = Fp - (j + 1) * PB, (j + 1) * PB
        if lookahead:
            first = pair_on and j % 2 == 0 and rest > PB and rest >= pair_min
            second = pair_on and j % 2 == 1 and rest > 0 and rest + PB >= pair_min
            br = "first of a pair" if first else "second of a pair" if second else "unpaired after pairs" if paired else "lookahead"
            paired = paired or first
            if rest > 0:
                out.append((br, "solve, first block", PB, PB, PB, 0))
                out.append((br, "update, block done ahead", PB, PB, PB, 1))
                if rest > PB:
                    out.append((br, "solve, rest of the row", PB, PB, rest - PB, 0))
                    if first:
                        out.append((br, "update, strip of the pair's second row", PB, PB, rest - PB, 0))
                        out.append((br, "update, block (j+2, j+2)", PB, PB, PB, 1))
                    elif second:
                        out.append((br, "update, K = 256", 2 * PB, rest, rest, 2))
                    else:
                        out.append((br, "update, behind the block done ahead", PB, rest, rest, 2))
            out.append((br, "Y, scale", PB, PB, width, 0))
            if first:
                out.append((br, "Y, next block row", PB, PB, width, 0))
            elif second:
                out.append((br, "Y, K = 256", 2 * PB, rest, width, 0))
            elif rest > 0:
                out.append((br, "Y, below", PB, rest, width, 0))
            continue
        br = "overlap" if overlap else "one stream"
        if rest > 0:
            out.append((br, "solve, row", PB, PB, rest, 0))
            out.append((br, "update, trailing", PB, rest, rest, 1))
        # (without overlap the substitution follows the whole factorisation: the same calls, later)
        out.append((br, "Y, scale", PB, PB, width, 0))
        if rest > 0:
            out.append((br, "Y, below", PB, rest, width, 0))
    return out


def chol_kernel(env):
    """launch_chol_diag: RR_CHOL_DIAG=0 the plain kernel, =1 the pipelined one, otherwise the sub-panel / MFMA kernel."""
    which = int(env["RR_CHOL_DIAG"]) if env.get("RR_CHOL_DIAG") is not None else 2
    return CHOL_KERNELS[which] if which in (0, 1) else CHOL_KERNELS[2]


def predicted_launches(F, env, route="pipeline"):
    """{kernel: launches} of one call at F columns under the switches env.  route: 'pipeline' (rr_posterior_dev), 'small' (the
    same with RR_POSDEF_SMALL=1 at F <= 1024), 'factor' / 'factor0' (rr_variance_factor_dev with form 1 / form 0)."""
    want = dict.fromkeys(KERNELS, 0)
    nblk = (F + PB - 1) // PB
    Fp = nblk * PB
    if route == "small":
        assert F <= 1024
        want["rr_posterior_coop_kernel"] = want["rr_posterior_rows_kernel"] = 1
        return want
    want[chol_kernel(env)] = nblk
    if route in ("factor", "factor0"):      # chol_upper_blocked: one stream, whole rows
        want["rr_reverse_pad_kernel"] = 1
        want["rr_ul_factor_f32_kernel" if route == "factor" else "rr_c64_to_c32_kernel"] = 1
        for j in range(nblk):
            rest = Fp - (j + 1) * PB
            if rest > 0:
                want[gemm_kernel(PB, PB, rest, 0, env)] += 1
                want[gemm_kernel(PB, rest, rest, 1, env)] += 1
        return want
    for _, _, K, M, N, uo in pipeline_calls(F, env):
        want[gemm_kernel(K, M, N, uo, env)] += 1
    want["rr_syrk_f64_kernel"] = 1                      # rr_launch_syrk_f64 on Y (Fp, Fp): nb = nblk column blocks,
    want["rr_syrk_f64_diag_kernel"] = 1 if nblk >= 2 else 0   # the diagonal tiles in their own kernel from two
    want["rr_posterior_rows_kernel"] = 1
    return want


# ---- exact data ---------------------------------------------------------------------------------------------------------
def _lowbit(a):
    """The value of the lowest set bit of every entry of a (nonzero entries only, flat)."""
    a = np.abs(np.asarray(a, dtype=np.float64).ravel())
    a = a[a != 0]
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    return np.ldexp((mi & -mi).astype(np.float64), e - 53), a


def _quantum(a):
    """The largest power of two that divides every entry of a."""
    low, _ = _lowbit(a)
    return float(low.min()) if low.size else 1.0


def _bits(a):
    """The largest number of significant bits over the entries of a."""
    low, v = _lowbit(a)
    return int((np.frexp(v)[1] - np.frexp(low)[1]).max()) + 1 if low.size else 0


def make_factor(F, seed, isolated=()):
    """(d, N) of U = diag(d) + N (module docstring).  isolated: [(k, d_k)] -- row and column k of N zero, d[k] = d_k."""
    rs = np.random.RandomState(seed)
    i = np.arange(F)
    lev = (i - F) % 3                      # the last column on the top level: a ragged last panel of one column is coupled
    elig = (i[:, None] < i[None, :]) & (lev[:, None] < lev[None, :])
    N = np.where(elig & (rs.random_sample((F, F)) < density(F)), rs.choice([-2.0, -1.0, 1.0, 2.0], size=(F, F)), 0.0)
    d = rs.choice(DVALS if F > 100 else DVALS_SMALL, size=F)
    for k, dk in isolated:
        N[k, :] = 0.0
        N[:, k] = 0.0
        d[k] = dk
    return d, N


def _pad(A, Fp):
    out = np.eye(Fp)
    out[:A.shape[0], :A.shape[1]] = A
    return out


def _check_sensitive(U, Uinv):
    """Module docstring, "Sensitivity"; U, U^-1 of F columns, padded with the identity here."""
    nblk = (U.shape[0] + PB - 1) // PB
    if nblk < 2:
        return
    Up, Yp = _pad(U, nblk * PB), _pad(Uinv, nblk * PB).T
    rs = np.random.RandomState(7)    # four pairs of vectors: one nonzero form is enough
    x, z = rs.randint(1, 4, size=(4, nblk, PB)).astype(np.float64), rs.randint(1, 4, size=(4, nblk, PB)).astype(np.float64)
    Ux = np.einsum("prab,vab->vpra", Up.reshape(nblk, PB, nblk, PB), x)     # U[p,a] x_a
    Uz = np.einsum("prab,vab->vpra", Up.reshape(nblk, PB, nblk, PB), z)
    Yz = np.einsum("prcb,vcb->vprc", Yp.reshape(nblk, PB, nblk, PB), z)     # Y[p,c] z_c
    uu = (np.einsum("vpra,vprb->vpab", Ux, Uz) != 0).any(axis=0)            # x^T U[p,a]^T U[p,b] z
    uy = (np.einsum("vpra,vprc->vpac", Ux, Yz) != 0).any(axis=0)
    for p in range(nblk):
        for a in range(p + 1, nblk):
            assert uu[p, a, a:].all(), ("U[p,a]^T U[p,b] vanishes", p, a)
            assert uy[p, a, :p + 1].all(), ("U[p,a]^T Y[p,c] vanishes", p, a)


BOUND_BITS = {}   # F: {sum: log2(bound / quantum)} of the last case made at F columns


def _check_exact(d, N, U, Uinv, C, G, b, iso):
    """Module docstring: every sum of the device's algorithm, divided by its quantum, stays below 2^53."""
    keep = np.ones(len(d), dtype=bool)
    keep[list(iso)] = False
    kk = np.ix_(keep, keep)
    Ua, Na, dk = np.abs(U[kk]), np.abs(N[kk]), d[keep]
    if dk.size:
        eye = np.eye(dk.size)
        Ma = Na / dk[:, None]
        A = (eye + Ma + Ma @ Ma) / dk[None, :]
        assert (np.abs(Uinv[kk]) <= A).all()
        qU, qI = _quantum(Ua), _quantum(Uinv[kk])
        B1 = Ua.T @ Ua
        B3 = eye + Na.T @ A.T
        bounds = {"Schur complements": 2 * B1.max() / qU ** 2,
                  "panel solves": (A.T @ B1).max() / (qI * qU ** 2),
                  "substitution, sums": B3.max() / (qU * qI),
                  "substitution, scaling": (A.T @ B3).max() / (qI ** 2 * qU),
                  "C = Y^T Y": (A @ A.T).max() / qI ** 2,
                  "m = C b / var": (np.abs(C[kk]) @ np.abs(b[keep])).max() / _quantum(C[kk])}
        BOUND_BITS[len(d)] = {k: round(float(np.log2(v)), 1) for k, v in bounds.items()}
        assert max(bounds.values()) < LIMIT, bounds
    nz = (G != 0) & (C != 0)
    if nz.any():
        lg, vg = _lowbit(G[nz])
        lc, vc = _lowbit(C[nz])
        assert ((np.frexp(vg)[1] - np.frexp(lg)[1]) + (np.frexp(vc)[1] - np.frexp(lc)[1]) + 2 <= 53).all()   # G o C is exact
        P = G * C
        assert np.abs(P).sum() / _quantum(P) < LIMIT
    if len(d) >= 64:
        assert _bits(C) > 24, _bits(C)


def make_case(F, seed=None, isolated=(), lower_pivot=None):
    """The inputs and the closed-form posterior of one factor.  lower_pivot = (k, by): iC[k, k] lowered by `by` afterwards
    (a matrix to be refused; no reference)."""
    d, N = make_factor(F, F if seed is None else seed, isolated)
    U = np.diag(d) + N
    rs = np.random.RandomState(F + 1)
    iL = rs.randint(1, 4, size=F).astype(np.float64)
    b = rs.randint(-3, 4, size=F).astype(np.float64)
    iC = U.T @ U
    if lower_pivot is not None:
        iC[lower_pivot[0], lower_pivot[0]] -= lower_pivot[1]
        G = (iC - np.diag(iL)) * VAR
        assert np.array_equal(G / VAR + np.diag(iL), iC)
        return {"F": F, "G": G, "b": b, "iL": iL}
    M = N / d[:, None]
    Uinv = (np.eye(F) - M + M @ M) / d[None, :]
    assert np.array_equal(U @ Uinv, np.eye(F))
    C = Uinv @ Uinv.T
    G = (iC - np.diag(iL)) * VAR
    assert np.array_equal(G / VAR + np.diag(iL), iC) and np.array_equal(C, C.T)
    _check_exact(d, N, U, Uinv, C, G, b, [k for k, _ in isolated])
    if not isolated:      # (an isolated last column of a one-column panel leaves that panel's blocks empty, as it must)
        _check_sensitive(U, Uinv)
    e = np.log2(d)
    assert np.array_equal(e, np.round(e))
    terms = np.cumsum(2.0 * np.log(d))
    case = {"F": F, "G": G, "b": b, "iL": iL, "C": C, "m": (C @ b) / VAR, "tr": float((G * C).sum()), "d": d,
            "logdet": 2.0 * float(e.sum()) * np.log(2.0), "logdet_tol": F * 2.0 ** -52 * max(1.0, float(np.abs(terms).max()))}
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=1)
def _big_case(F):
    return make_case(F)


@functools.lru_cache(maxsize=3)
def _small_case(F):
    return make_case(F)


def _case(F):
    """Made once and read-only (the one of 4400 columns, whose reference is a few seconds of matrix products, in a cache of its own)."""
    return (_big_case if F > 2048 else _small_case)(F)


# ---- running the device -------------------------------------------------------------------------------------------------
def _device():
    from revrand_amd import _hip
    return _hip.get_device()


def run_posterior(case, det=False):
    """One rr_posterior_dev on the case's inputs: (rc, m, diag C, [log|iC|, sum(G o C), min pivot], C, problems) -- C from a
    buffer one row longer than F x F and prefilled with SENTINEL; problems: what the call did to memory that is not its own."""
    from revrand_amd import _hip
    dev, F = _device(), case["F"]
    inp = np.concatenate((case["G"].ravel(), case["b"]))
    acc = dev.upload_vector(inp)
    dC = dev.upload_vector(np.full(F * F + F, SENTINEL, dtype=np.uint64))
    m, dg, scal = np.full(F, np.nan), np.full(F, np.nan), np.full(3, np.nan)
    iL = np.ascontiguousarray(case["iL"], dtype=np.float64)
    was = dev.set_deterministic(det)
    try:
        pG, pb = _hip.ctypes.c_void_p(acc.ptr.value), _hip.ctypes.c_void_p(acc.ptr.value + F * F * 8)
        rc = dev.lib.rr_posterior_dev(dev.ctx, F, pG, pb, iL.ctypes.data_as(_hip.ctypes.c_void_p), VAR, dC.ptr,
                                      m.ctypes.data_as(_hip.ctypes.c_void_p), dg.ctypes.data_as(_hip.ctypes.c_void_p),
                                      scal.ctypes.data_as(_hip.ctypes.c_void_p))
        dev.sync()
        out = dev.download(dC, (F * F + F,), np.uint64)
        back = dev.download(acc, (F * F + F,), np.float64)
    finally:
        dev.set_deterministic(was)
        acc.free()
        dC.free()
    problems = []
    if not (out[F * F:] == SENTINEL).all():
        problems.append("the row behind C was written")
    if not np.array_equal(back, inp):
        problems.append("G or b changed on the device")
    return rc, m, dg, scal, out[:F * F].view(np.float64).reshape(F, F), problems


def mismatches(case, det=False, what=""):
    """[] or one line per output of rr_posterior_dev that is not the closed form's, bit for bit."""
    from revrand_amd import _hip
    rc, m, dg, scal, C, bad = run_posterior(case, det)
    what = "%sF = %d%s" % (what, case["F"], " det" if det else "")
    if rc != 0:
        return ["%s: rc = %d (%s)" % (what, rc, _hip.load_library().rr_last_error().decode())]
    for name, got, want in (("C", C, case["C"]), ("C^T", C.T, case["C"]), ("m", m, case["m"]), ("diag C", dg, case["C"].diagonal())):
        ne = ~(got == want)        # (a sentinel left in C is a NaN: unequal)
        if ne.any():
            first = tuple(int(v) for v in np.argwhere(ne)[0])
            bad.append("%s: %d of %d differ, first at %s (panel %s): %r for %r" % (name, int(ne.sum()), ne.size, first,
                       tuple(v // PB for v in first), float(got[first]), float(want[first])))
    if scal[1] != case["tr"]:
        bad.append("sum(G o C): %r for %r" % (float(scal[1]), case["tr"]))
    if not abs(scal[0] - case["logdet"]) <= case["logdet_tol"]:
        bad.append("log|iC|: %r for %r (tolerance %g)" % (float(scal[0]), case["logdet"], case["logdet_tol"]))
    if scal[2] != case["d"].min():
        bad.append("smallest pivot: %r for %r" % (float(scal[2]), float(case["d"].min())))
    return ["%s: %s" % (what, b) for b in bad]


def refused(case, det=False):
    """[] if rr_posterior_dev refuses the matrix as it must, else what it did instead."""
    from revrand_amd import _hip
    rc, _, _, _, _, bad = run_posterior(case, det)
    if rc != _hip.RR_ERR_NOT_POSDEF:
        bad.append("rc = %d, not RR_ERR_NOT_POSDEF" % rc)
    elif b"not safely positive definite" not in _hip.load_library().rr_last_error():
        bad.append("the error message does not say why")
    return ["F = %d, to be refused: %s" % (case["F"], b) for b in bad]


def both_modes(case, what=""):
    """The default mode, and the deterministic one twice (the slab path must run; the same bits follow from `==`)."""
    return mismatches(case, False, what) + mismatches(case, True, what) + mismatches(case, True, what + "again, ")


class _Small(object):
    """RR_POSDEF_SMALL (read per call) for the duration of a block."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.saved = os.environ.pop("RR_POSDEF_SMALL", None)
        if self.on:
            os.environ["RR_POSDEF_SMALL"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("RR_POSDEF_SMALL", None)
        if self.saved is not None:
            os.environ["RR_POSDEF_SMALL"] = self.saved


# ---- tests: the data and the route table (no device) ---------------------------------------------------------------------
@pytest.mark.parametrize("F", sorted(set(PIPELINE_F + SMALL_F + CHILD_F)))
def test_data_is_exact_in_any_summation_order(F):
    """make_case's own assertions (U Uinv == I, the bounds of `_check_exact`, `_check_sensitive`) at every size the device
    tests use; and the bounds have teeth: the same check refuses a factor whose entries need too many bits."""
    case = _case(F)
    assert case["C"].shape == (F, F) and np.array_equal(case["C"], case["C"].T)
    if F == 300:
        d, N = make_factor(F, F)
        N = N * (1.0 + 2.0 ** -26)            # 27-bit entries: the products no longer fit
        U = np.diag(d) + N
        with pytest.raises(AssertionError):
            M = N / d[:, None]
            Uinv = (np.eye(F) - M + M @ M) / d[None, :]
            _check_exact(d, N, U, Uinv, Uinv @ Uinv.T, (U.T @ U - np.eye(F)) * VAR, case["b"], [])


@pytest.mark.parametrize("F", REFUSAL_F)
def test_threshold_and_factor_data_is_exact(F):
    """The same assertions for the matrices of the threshold test (one isolated pivot of 2^-16 at each of `_refusal_indices`;
    the refused ones have no reference) and for the prediction factor's, which are exact in float32."""
    for k in _refusal_indices(F):
        ok, low, zero, neg = _refusal_cases(F, k)
        assert ok["C"][k, k] == 2.0 ** 32 and ok["d"].min() == 2.0 ** -16 > CHOLTHRESH > 2.0 ** -17
        assert zero["G"][k, k] < _case(F)["G"][k, k] and neg["G"][k, k] == zero["G"][k, k] - VAR
    if F == REFUSAL_F[0]:
        for Ff in FACTOR_F:
            factor_case(Ff)
        for Ff in FACTOR0_F:
            factor0_case(Ff)


def test_cases_cover_every_route():
    """From the restated rules: the in-process sizes and the child processes' variants reach every branch of the schedule,
    the paired branches with an odd panel left over and with none, and -- for every call site of rr_launch_gemm_tn_f64 -- both
    kernels where the site's shapes can take both (a K = 256 product and a trailing update of more than one tile never take
    the K = 128 kernel; with RR_GEMM64_K128=0 nothing does)."""
    runs = [(F, {}) for F in PIPELINE_F] + [(F, v) for v in VARIANTS for F in CHILD_F]
    branches, arms = {}, {}
    for F, env in runs:
        for br, site, K, M, N, uo in pipeline_calls(F, env):
            branches.setdefault(br, (F, variant_id(env)))
            arms.setdefault((site, gemm_kernel(K, M, N, uo, env)), (F, variant_id(env)))
    for k in sorted(branches):
        print("%-24s %s" % (k, branches[k]))
    assert set(branches) == {"one stream", "overlap", "lookahead", "first of a pair", "second of a pair", "unpaired after pairs"}
    sites = {s for s, _ in arms}
    never_k128 = {"update, K = 256", "Y, K = 256", "update, behind the block done ahead"}
    for s in sorted(sites):
        assert (s, "rr_gemm_tn_f64_kernel") in arms, s
        assert (s in never_k128) != ((s, "rr_gemm_tn_f64_k128_kernel") in arms), s
    # ... and by the default switches alone, in process: every branch but the two that need a smaller RR_POSDEF_PAIR_MIN
    # is reached by a size below 4400, and 4400 is the smallest F whose first panel is paired by default
    dflt = {br for F in PIPELINE_F if F <= 1280 for br, *_ in pipeline_calls(F, {})}
    assert dflt == {"one stream", "overlap", "lookahead"}
    assert {br for br, *_ in pipeline_calls(4400, {})} == {"first of a pair", "second of a pair", "unpaired after pairs"}
    assert [br for br, site, *_ in pipeline_calls(4400, {}) if site == "Y, scale"][:5] == ["first of a pair", "second of a pair"] * 2 + ["unpaired after pairs"]
    assert "first of a pair" not in {br for br, *_ in pipeline_calls(4096, {})}
    # the tile kernel on a one-tile trailing update with upper_only = 2 never happens (rest > 128 there): the rule's last
    # clause is about upper_only = 1
    assert all(M > PB for F, env in runs for _, _, K, M, N, uo in pipeline_calls(F, env) if uo == 2)
    # all panels paired: an odd panel left over behind the pairs (5, 9 panels: 640, 1153 -- the last panel can never be
    # a pair's first) and none (4, 10 panels)
    pm = {"RR_POSDEF_PAIR_MIN": "256"}
    tail = {F: [br for br, site, *_ in pipeline_calls(F, pm) if site == "Y, scale"] for F in CHILD_F}
    assert tail[640][-3:] == ["first of a pair", "second of a pair", "unpaired after pairs"] and tail[640].count("first of a pair") == 2
    assert tail[512] == ["first of a pair", "second of a pair", "unpaired after pairs", "unpaired after pairs"]
    assert tail[1280] == tail[1153] == ["first of a pair", "second of a pair"] * 4 + ["unpaired after pairs"] * 2
    assert tail[384] == ["first of a pair", "second of a pair", "unpaired after pairs"]
    pm = {"RR_POSDEF_PAIR_MIN": "512"}
    tail = [br for br, site, *_ in pipeline_calls(1280, pm) if site == "Y, scale"]
    assert tail[:6] == ["first of a pair", "second of a pair"] * 3 and set(tail[6:]) == {"unpaired after pairs"}
    # a switch that changes counts and no kernel's name must change the prediction somewhere, or its census proves nothing:
    # one stream and no look-ahead lose the look-ahead's one-tile launches (the same counts for both: what differs is the
    # stream), pairing changes the counts wherever it pairs, and RR_POSDEF_PAIR=0 takes that back
    default = [predicted_launches(F, {}) for F in CHILD_F]
    for v in ({"RR_POSDEF_OVERLAP": "0"}, {"RR_POSDEF_LOOKAHEAD": "0"}, {"RR_POSDEF_PAIR_MIN": "256"}, {"RR_POSDEF_PAIR_MIN": "512"}):
        assert v in VARIANTS and [predicted_launches(F, v) for F in CHILD_F] != default, v
    assert [predicted_launches(F, {"RR_POSDEF_PAIR_MIN": "256"}) for F in CHILD_F] != [predicted_launches(F, {"RR_POSDEF_PAIR_MIN": "512"}) for F in CHILD_F]
    assert [predicted_launches(F, {"RR_POSDEF_PAIR": "0", "RR_POSDEF_PAIR_MIN": "256"}) for F in CHILD_F] == default


# ---- tests: the pipeline, in process ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F", PIPELINE_F)
def test_pipeline_is_exact(F):
    """One, two and three to ten panels (full, ragged, one column into the next panel), and the default pairing at F = 4400:
    C, C^T, m, diag C, sum(G o C) and the smallest pivot bit for bit, log|iC| to its bound; nothing written behind C, G and b
    untouched; in deterministic mode twice."""
    assert both_modes(_case(F)) == []


@gpu
def test_scratch_follows_the_size():
    """1280 -> 300 -> 1280 -> 300 columns: the work space (sized exactly, Fp x Fp) is released and made again each time."""
    bad = []
    for F in (1280, 300, 1280, 300):
        bad += mismatches(_case(F))
    assert bad == []


@gpu
@pytest.mark.parametrize("F", SMALL_F)
def test_cooperative_kernel_is_exact(F):
    """RR_POSDEF_SMALL=1: factor, inverse and C in one cooperative launch (plain f64 FMAs out of LDS), on the same data."""
    with _Small(True):
        bad = both_modes(_case(F), "small, ")
    assert bad == []


def _refusal_indices(F):
    """Column 5, a column of panel nblk // 2 and the last column: the first, a middle and the ragged last panel where there
    are three (700: panels 0, 3, 5; 1153: 0, 5 and the one-column panel 9); at 200 columns the first and twice the second,
    ragged, panel (5, 133, 199); at 100 three columns of the only one (5, 77, 99)."""
    mid = (F + PB - 1) // PB // 2 * PB
    return sorted({5, mid + 77 % (F - mid), F - 1})


@functools.lru_cache(maxsize=3)
def _refusal_cases(F, k):
    return (make_case(F, isolated=[(k, 2.0 ** -16)]), make_case(F, isolated=[(k, 2.0 ** -17)], lower_pivot=(k, 0.0)),
            make_case(F, lower_pivot=(k, make_factor(F, F)[0][k] ** 2)), make_case(F, lower_pivot=(k, make_factor(F, F)[0][k] ** 2 + 1.0)))


@gpu
@pytest.mark.parametrize("F,small", [(F, s) for F in REFUSAL_F for s in (False, True) if F <= 1024 or not s],
                         ids=lambda v: {False: "pipeline", True: "small"}.get(v, str(v)) if isinstance(v, bool) else str(v))
def test_threshold_is_exact_and_a_refusal_leaves_nothing_behind(F, small):
    """An isolated pivot d_k = 2^-16 (above CHOLTHRESH = 1e-5) is accepted, with C[k, k] = 2^32 and everything else exact;
    d_k = 2^-17 is refused, and so are a pivot of exactly 0 and of exactly -1 (iC[k, k] lowered by d_k^2 and d_k^2 + 1; k not
    isolated).  k as `_refusal_indices` places it: in the first, a middle and the ragged last panel at 700 and 1153 columns, in
    both panels at 200, three times in the only panel at 100.  After every refusal a good matrix of the same size is
    exact straight away: nothing of the refused call is left running on the second or third stream."""
    bad = []
    with _Small(small):
        for k in _refusal_indices(F):
            ok, low, zero, neg = _refusal_cases(F, k)
            assert ok["C"][k, k] == 2.0 ** 32 and ok["d"].min() == 2.0 ** -16 > CHOLTHRESH > 2.0 ** -17
            bad += mismatches(ok, what="d[%d] = 2^-16, " % k)
            for case in (low, zero, neg):
                bad += refused(case) + mismatches(_case(F), what="after a refusal at %d, " % k)
    assert bad == []


# ---- tests: the prediction factor ---------------------------------------------------------------------------------------
def run_factor(Cin):
    """(B (Fb, Fb) float32, form) of DeviceCovariance(Cin).factor()."""
    from revrand_amd import _hip
    dev, F = _device(), Cin.shape[0]
    cov = _hip.DeviceCovariance(dev, Cin)
    try:
        B, form = cov.factor()
        Fb = (F + 255) // 256 * 256
        dev.sync()
        return dev.download(B, (Fb, Fb), np.float32), form
    finally:
        cov.free()


def factor_case(F, isolated=()):
    """(C = M M^T, M): M = J U^T J upper triangular, so that J C J = U^T U and the blocked Cholesky returns U bit for bit."""
    d, N = make_factor(F, F, isolated)
    U = np.diag(d) + N
    M = np.ascontiguousarray(U.T[::-1, ::-1])
    C = M @ M.T
    assert np.array_equal(np.ascontiguousarray(C[::-1, ::-1]), U.T @ U) and np.array_equal(np.triu(M), M)
    assert np.array_equal(M.astype(np.float32).astype(np.float64), M)
    return C, M


FACTOR0_F = [100, 300]


def factor0_case(F):
    """(C, the float32 (Fb, Fb) buffer of form 0): one isolated d = 2^-24 puts the factor's diagonal more than 1e7 apart.
    (Its pivot 4^-24 lies outside the range k = -17 .. 8 of the square root's host test; only the decision for form 0 reads
    that square root -- anything within a factor of five of 2^-24 decides the same -- and the buffer compared here is a
    conversion of C, not of the factor.)"""
    k = F // 3
    C, M = factor_case(F, isolated=[(F - 1 - k, 2.0 ** -24)])
    assert M[k, k] == 2.0 ** -24 < 1e-7 * np.abs(M.diagonal()).max() and C[k, k] == 2.0 ** -48
    want = np.zeros(((F + 255) // 256 * 256,) * 2)
    want[:F, :F] = np.triu(C, 1) * 2.0 + np.diag(C.diagonal())
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return C, want.astype(np.float32)


def factor_mismatches(F):
    C, M = factor_case(F)
    B, form = run_factor(C)
    want = np.zeros(B.shape, dtype=np.float32)
    want[:F, :F] = M
    bad = [] if form == 1 else ["F = %d: form %d" % (F, form)]
    if not np.array_equal(B, want):
        bad.append("F = %d: %d entries of the factor differ" % (F, int((B != want).sum())))
    return bad


@gpu
@pytest.mark.parametrize("F", FACTOR_F)
def test_variance_factor_is_exact(F):
    """rr_variance_factor_dev (rr_reverse_pad_kernel, chol_upper_blocked -- the single-stream driver of the same kernels --,
    rr_ul_factor_f32_kernel): the float32 (Fb, Fb) factor is M in its top-left F x F, zero elsewhere, form 1.  (`factor_case`
    asserts what this needs: J C J == U^T U and M exact in float32; the bounds on U^T U are those of the same factor's
    posterior case, asserted on the host at every size.)"""
    assert factor_mismatches(F) == []


@gpu
@pytest.mark.parametrize("F", FACTOR0_F)
def test_variance_factor_falls_back_to_the_quadratic_form(F):
    """A factor whose diagonal spans more than 1e7 (one isolated d = 2^-24 against 4 or 8): form 0, the buffer holds the upper
    triangle of C with doubled off-diagonal entries -- all of them exact in float32 (asserted)."""
    C, want = factor0_case(F)
    B, form = run_factor(C)
    assert form == 0
    assert np.array_equal(B, want)


# ---- the switches read once per process: one child process each ---------------------------------------------------------
def clear_switches(keep):
    """(first thing in a child process, before the library reads them) no posterior switch but the variant's own."""
    for k in SWITCHES:
        if k not in keep:
            os.environ.pop(k, None)


def variant_child():
    """CHILD_F in both modes under this process' switches: the list of mismatches.  With RR_POSDEF_EARLY_CHECK also a
    refusal (the pivots are asked for before C = Y^T Y is queued) and the good matrix behind it."""
    bad = []
    for F in CHILD_F:
        bad += both_modes(_case(F))
    if os.environ.get("RR_POSDEF_EARLY_CHECK") is not None:
        k = 5 * PB + 3
        bad += refused(make_case(700, isolated=[(k, 2.0 ** -17)], lower_pivot=(k, 0.0))) + mismatches(_case(700), what="after a refusal, ")
    return bad


CHILD_CODE = ("import test_gpu_posterior_exact as P\nP.clear_switches(%r)\n")


@gpu
@pytest.mark.parametrize("variant", [{}] + VARIANTS, ids=variant_id)
def test_switch_variants_are_exact(variant):
    """One stream; no look-ahead; every panel paired (4, 5, 9 and 10 panels: an odd panel left over and none); pairs first and
    an unpaired tail; pairing switched off; the early pivot check; the plain and the pipelined diagonal-block kernels; no
    K = 128 kernel -- each in a child process of its own (and the default switches in one, whose time sizes the limit),
    one after another, none started after one that failed or hung."""
    from test_gpu_gram_exact import guarded_child
    code = CHILD_CODE % (sorted(variant),) + "print('PRESULT', json.dumps(P.variant_child()))\n"
    assert guarded_child("the posterior under %s" % variant_id(variant), code, variant, "PRESULT", timeout=CHILD_TIMEOUT) == []


# ---- which kernel ran (the bounds-checking build's launch counts; tests/test_debug_builds.py) ---------------------------
CENSUS_SMALL_F = [100, 512, 1000]
CENSUS_FACTOR_F = [100, 129, 700]


CENSUS_F = CHILD_F + [1, 300]


def census_labels():
    """The calls of `census()`, in its order."""
    return (["pipeline(%d)%s" % (F, det) for F in CENSUS_F for det in ("", " det")] + ["small(%d)" % F for F in CENSUS_SMALL_F] +
            ["factor(%d)" % F for F in CENSUS_FACTOR_F] + ["factor0(300)"])


def census():
    """Launches of each posterior kernel per call under a library that counts them (rr_debug_kernel_launches), next to the
    restated rules' prediction for this process' switches: [(label, {kernel: launches}, {kernel: predicted})].  Every call
    is also checked for exactness -- a census of wrong results would be worth little."""
    dev = _device()
    lib = dev.lib
    assert lib.rr_debug_kernel_launches(None) == 0
    env, out = dict(os.environ), []

    def counted(label, call, want):
        dev.sync()
        lib.rr_debug_kernel_launches(None)
        bad = call()
        dev.sync()
        got = {k: int(lib.rr_debug_kernel_launches(k.encode())) for k in KERNELS}
        out.append((label, got, want, bad))

    for F in CENSUS_F:
        for det in (False, True):
            counted("pipeline(%d)%s" % (F, " det" if det else ""), lambda: mismatches(_case(F), det), predicted_launches(F, env))
    for F in CENSUS_SMALL_F:
        with _Small(True):
            counted("small(%d)" % F, lambda: mismatches(_case(F)), predicted_launches(F, env, "small"))
    for F in CENSUS_FACTOR_F:
        counted("factor(%d)" % F, lambda: factor_mismatches(F), predicted_launches(F, env, "factor"))

    def form0():
        C, want = factor0_case(300)
        B, form = run_factor(C)
        return [] if form == 0 and np.array_equal(B, want) else ["form %d, or not the doubled upper triangle" % form]
    counted("factor0(300)", form0, predicted_launches(300, env, "factor0"))
    assert [row[0] for row in out] == census_labels()
    return out
