"""Every kernel route of the Gram G = Phi^T Phi (+ Phi^T y, y^T y) against exact references, bit for bit.

rr_launch_syrk_f32 (rr_rff.hip) picks its kernels from the padded shape, the rider column and the CU count:
the 128 x 128 small kernel, or the 256 x 256 main kernel with or without its diagonal tiles (rr_syrk_f32_diag16_kernel),
with or without the ragged-last-block kernel and the XCD tile map, each with a K-split count of its own;
rr_launch_syrk_f64 (the same file) has the pair rr_syrk_f64_kernel / rr_syrk_f64_diag_kernel, rr_launch_syrk_bf16
(rr_syrk16.hip) the conversion rr_split_bf16_kernel and rr_syrk_b16w4_kernel<3 | 4>.  `f32_route`, `f64_route` and
`b16_route` restate those rules (not the split-count searches: a case that needs a known K-split geometry forces it
with RR_GRAM_ROWS_PER_SPLIT, read per call); the cases below are chosen so that, on the MI355X's 256 CUs, they reach
every route, and `test_cases_cover_every_route` checks that at the CU count of the device it runs on.

Three data sets make every route's result exact whatever its summation order, K-split or atomics:

* f32 engine: Phi integer in [-3, 3], y integer in [-2, 2].  An f32 accumulator sums integer products over one K-split
  of at most 32 768 rows; the largest entry of |[Phi | y]|^T |[Phi | y]| over such rows is on its diagonal (Cauchy-Schwarz),
  so `_check_f32_exact` asserts that the column sums of squares of any two adjacent 32 768-row chunks (a K-split spans
  at most two) stay below 2^24.  The f64 atomics across K-splits, the deterministic slabs and their ordered reduction
  then add integers below 2^53.
* f64 pair: integers in [-1000, 1000], products up to 10^6, column sums of squares below 2^53 (asserted): a path that
  narrowed to f32 anywhere would fail.
* split 16-bit engines: v = h + l with h in {-2, .., 2}, l in {0, +-2^-10} and l = 0 where h = 0.  |l| is below half a
  bf16 ulp of h, so the round-to-nearest-even split gives hi = h, lo = l (`_bf16_split`, a NumPy emulation, asserts it).
  bf16x3 must return h^T h + h^T l + l^T h and bf16x4 that plus l^T l, evaluated in float64.  All products of one entry
  share one f32 accumulator per K-split, so its partial sums must fit 24 bits: quantum 2^-10 for x3 -- sum |v||v'| < 2^14,
  which holds for ANY density over a 1024-row split (<= 1024 (2 + 2^-10)^2 < 4101), so x3 runs dense (`_split_dense`) at the
  launcher's own splits -- and quantum 2^-20 for x4: sum |v||v'| < 16 per K-split, largest on the diagonal (sum v^2).  Over
  a 1024-row split that allows three nonzeros per column, too sparse for a dropped k-block to show; so the x4 cases force
  64-row splits (RR_GRAM_ROWS_PER_SPLIT=64, one 64-row k-step pair per workgroup) on data with at most three nonzeros
  per column in every aligned 64-row block (`_split_sparse`, 4.7 % dense, 3 (2 + 2^-10)^2 < 12.1 < 16 -- asserted).  The same
  sparse data also runs x3 at 64-row and at the launcher's splits, and x4 runs at the launcher's splits on data with one
  nonzero per column and 1100 rows (`_split_sparse_long`: every 16-row k-step still holds nonzeros of some columns, so a
  dropped one shows on the diagonal).  fp16x3 on a host-put matrix falls back to the bf16x3
  split and must give bf16x3's bits.

The widths 512 + w of the ragged-block cases and 700 of the K-split cases take the small kernel at 3001 / 4000 rows on
256 CUs (ldp = 768: 6 tiles x 3 or 4 < 256); they stay as exactness cases, and the same cases 512 columns wider
(ldp = 1280 > 1024: never small) are the ones that reach the ragged kernel and the main kernel's K-splits.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

EXACT = 1 << 24
SYRK_KERNELS = ["rr_syrk_f32_small_kernel", "rr_syrk_f32_kernel", "rr_syrk_f32_flat_kernel", "rr_syrk_f32_flatstag_kernel",
                "rr_syrk_f32_buf_kernel", "rr_syrk_f32_ragged_kernel", "rr_syrk_f32_diag16_kernel", "rr_syrk_f32_diag_kernel",
                "rr_syrk_f32_merged_kernel", "rr_syrk_det_reduce_kernel", "rr_syrk_b16w4_kernel", "rr_split_bf16_kernel",
                "rr_syrk_f64_kernel", "rr_syrk_f64_diag_kernel", "rr_fm_set_column_kernel", "rr_fm_gemv_t_kernel"]
# read once per process (rr_syrk_switches, rr_syrk_plan.h): each runs in a child process of its own
AB_VARIANTS = [{"RR_SYRK_SMALL": "0"}, {"RR_SYRK_NO_DIAG16": "1"}, {"RR_SYRK_DIAG_KB": "64"}, {"RR_SYRK_MERGE_DIAG": "1"},
               {"RR_SYRK_STAGGER": "0"}, {"RR_SYRK_STAGGER": "1"}, {"RR_SYRK_STAGGER": "2"}, {"RR_SYRK_SPLIT_SEARCH": "0"}]
AB_NAMES = sorted({k for v in AB_VARIANTS for k in v})
PER_CALL = ("RR_GRAM_ROWS_PER_SPLIT", "RR_GRAM_NO_TILE_MAP", "RR_SYRK_NO_DIAG_KERNEL")


# ---- the route tables ---------------------------------------------------------------------------------------------------
def _up(n, m):
    return (n + m - 1) // m * m


def f32_route(rows, F, rider, cu, env=None):
    """rr_launch_syrk_f32's kernel choice for `rows` feature rows (padded to 32 by rr_featmat_begin / rr_dense_gram) of F
    columns, with or without the rider column, at `cu` compute units; env: the switches in force (default os.environ)."""
    env = os.environ if env is None else env
    rows_pad, ldp = _up(rows, 32), _up(F, 256)                                       # rr_featmat_create's ld, rr_featmat_begin's rows_pad
    nb_all = ldp // 256                                                              # nb_all
    big_tiles = nb_all * (nb_all + 1) // 2                                           # big_tiles
    small_off = env.get("RR_SYRK_SMALL") is not None and int(env["RR_SYRK_SMALL"]) == 0   # small_off
    r = {"engine": "f32", "ldp": ldp, "nb_all": nb_all, "rider": bool(rider)}
    if not small_off and ldp <= 1024 and big_tiles * (_up(rows_pad, 1024) // 1024) < cu:    # the small kernel's condition
        r.update(kind="small", od=0, rg=0, nb=ldp // 128, w_last=None, use_map=False)
        r["ntiles"] = r["nb"] * (r["nb"] + 1) // 2                                   # nbs, nt
        return r
    od = 1 if nb_all >= 2 and not env.get("RR_SYRK_NO_DIAG_KERNEL") else 0           # od
    w_last = F + (1 if rider else 0) - 256 * (nb_all - 1)                            # w_last
    rg = 1 if od and nb_all >= 3 and w_last <= 192 else 0                            # rg
    nb = nb_all - rg                                                                 # nb
    ntiles = nb * (nb - 1) // 2 if od else nb * (nb + 1) // 2                        # ntiles
    use_map = ntiles % 8 == 0 and not env.get("RR_GRAM_NO_TILE_MAP")                 # use_map
    r.update(kind="main", od=od, rg=rg, nb=nb, w_last=w_last, ntiles=ntiles, use_map=use_map)
    return r


def f64_route(F, env=None):
    """rr_launch_syrk_f64 (rr_rff.hip): 128-column blocks, the diagonal tiles in their own kernel from two."""
    env = os.environ if env is None else env
    nb = _up(F, 128) // 128                                                          # nb
    od = 1 if nb >= 2 and not env.get("RR_SYRK_NO_DIAG_KERNEL") else 0               # od
    return {"engine": "f64", "kind": "f64", "nb": nb, "od": od, "ntiles": nb * (nb - 1) // 2 if od else nb * (nb + 1) // 2}


def b16_route(F, env=None):
    """rr_launch_syrk_bf16 (rr_syrk16.hip): every upper tile in one kernel, its own tile map."""
    env = os.environ if env is None else env
    nb = _up(F, 256) // 256                                                          # nb
    ntiles = nb * (nb + 1) // 2                                                      # ntiles
    return {"engine": "b16", "kind": "b16", "nb": nb, "ntiles": ntiles,
            "use_map": ntiles % 8 == 0 and not env.get("RR_GRAM_NO_TILE_MAP")}       # use_map


def takes_rider(F, with_y, engine="f32"):
    """rr_featmat_gram (rr_featmat.hip), `rider`: y rides in the first pad column of the f32 engine's SYRK, if there is one."""
    return bool(with_y) and engine == "f32" and F % 256 != 0


def route_name(r):
    if r["kind"] == "small":
        return "small"
    if r["kind"] == "main":
        return "main" + ("+ragged" if r["rg"] else "") + ("+diag16" if r["od"] else "")
    return r["kind"]


def predicted_launches(r, with_y, det, env=None, featmat=True):
    """{kernel: launches} of one Gram on route r (the launches at the end of rr_launch_syrk_f32, with its A/B switches)."""
    env = os.environ if env is None else env
    want = dict.fromkeys(SYRK_KERNELS, 0)
    if featmat and with_y and r["engine"] != "f64":
        if r.get("rider"):
            want["rr_fm_set_column_kernel"] = 2          # y in, zero again
        else:
            want["rr_fm_gemv_t_kernel"] = 1
    if r["engine"] == "b16":
        want["rr_split_bf16_kernel"] = want["rr_syrk_b16w4_kernel"] = 1
        return want
    if det:
        want["rr_syrk_det_reduce_kernel"] = 1
    if r["engine"] == "f64":
        want["rr_syrk_f64_kernel"] = 1 if r["ntiles"] > 0 else 0
        want["rr_syrk_f64_diag_kernel"] = r["od"]
        return want
    if r["kind"] == "small":
        want["rr_syrk_f32_small_kernel"] = 1
        return want
    mode = int(env["RR_SYRK_STAGGER"]) if env.get("RR_SYRK_STAGGER") else 3                    # syrk_mode
    merge = env.get("RR_SYRK_MERGE_DIAG") is not None and int(env["RR_SYRK_MERGE_DIAG"]) != 0  # merge_diag
    no_diag16 = env.get("RR_SYRK_NO_DIAG16") is not None                                       # no_diag16
    if merge and r["od"] and not r["rg"] and r["ntiles"] > 0 and mode == 3 and not no_diag16:  # the merged launch's condition
        want["rr_syrk_f32_merged_kernel"] = 1
        return want
    if r["ntiles"] > 0:
        want[{0: "rr_syrk_f32_flat_kernel", 1: "rr_syrk_f32_flatstag_kernel", 2: "rr_syrk_f32_buf_kernel"}
             .get(mode, "rr_syrk_f32_kernel")] = 1                                             # if (ntiles > 0): one of four
    want["rr_syrk_f32_ragged_kernel"] = r["rg"]
    if r["od"]:
        want["rr_syrk_f32_diag_kernel" if no_diag16 else "rr_syrk_f32_diag16_kernel"] = 1      # if (od)
    return want


# ---- the cases (rows, F, with y) ----------------------------------------------------------------------------------------
SMALL_F = [1, 100, 255, 256, 300, 1000, 1024]
SMALL_ROWS = [37, 1000, 5003]
BIG_CASES = [(262149, 200),   # main kernel alone (nb_all = 1): the narrow model on a large data set
             (87101, 500),    # main + diag16, nb_all = 2
             (3001, 1100),    # nb_all = 5, w_last = 76 (+ 1): main + ragged + diag16
             (3001, 1280)]    # nb_all = 5, w_last = 256: main + diag16, Phi^T y by the gemv kernel
RAGGED_W = [1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193]
RAGGED_W_Y = [31, 32, 127, 128, 191, 192]  # + the rider: w_last = w + 1, so 192 leaves the ragged kernel
RAGGED_BASE = [512, 1024]     # ldp = 768 (the small kernel at 3001 rows on 256 CUs) and ldp = 1280 (the ragged kernel)
RAGGED_ROWS = 3001
MAP_ROWS = 1000
MAP_CASES = [(4096, {}), (4096, {"RR_GRAM_NO_TILE_MAP": "1"}), (4100, {}), (4100, {"RR_GRAM_NO_TILE_MAP": "1"}),
             (4096, {"RR_SYRK_NO_DIAG_KERNEL": "1"}), (3840, {"RR_SYRK_NO_DIAG_KERNEL": "1"})]
KSPLIT_F = [300, 700, 1100, 1250]
KSPLIT_ROWS = 4000
KSPLIT_RPS = ["32", "64", "96", "1024", "4096", None]
CONTRACT_CASES = [(1000, 300, True), (1000, 512, True), (3001, 1100, True), (3001, 1280, True), (3001, 1100, False),
                  (1000, 4100, False)]
DET_CASES = [(1000, 300, True), (5003, 1024, True), (262149, 200, True), (87101, 500, True), (3001, 1100, True),
             (3001, 1280, True), (3001, 1024 + 192, True), (1000, 4100, False), (1000, 4096, False)]
REUSE_F = [700, 512, 1100]
REUSE_ROWS = [1000, 37, 300, 1, 1000]
DENSE32_CASES = [(1003, 300), (3001, 1100), (87101, 500)]
F64_F = [100, 130, 300, 1030]
F64_ROWS = [1, 17, 500, 5003]
SPLIT_DENSE = [(1000, 100), (3001, 100), (1000, 300), (3001, 300), (1000, 700), (3001, 700), (1000, 3840), (1000, 4096),
               (2016, 300)]   # 2016 = 32 (mod 64): the conversion pads to 64 rows with zeros
# one case per route at <= 5003 rows for the child processes of the A/B variants (+ a row count that is / is not a
# multiple of 64 after padding for RR_SYRK_DIAG_KB=64, and both tile-map widths: the flat variants read the map too)
AB_CASES = [(1000, 300, True), (5003, 200, True), (3001, 500, True), (3001, 1100, True), (3001, 1280, True),
            (3030, 1100, False), (3030, 1280, True), (3001, 1024 + 193, False), (200, 4096, False), (200, 4100, False)]


def route_cases(cu):
    """(label, route) of every Gram the tests below run with the default switches or the per-call ones."""
    out = []

    def f32(kind, rows, F, y, env=None):
        r = f32_route(rows, F, takes_rider(F, y), cu, env or {})
        r["with_y"] = bool(y)     # without the rider, Phi^T y comes from rr_fm_gemv_t_kernel
        out.append(("%s%s" % (kind, (rows, F, y) + ((sorted(env),) if env else ())), r))

    for F in SMALL_F:
        for rows in SMALL_ROWS:
            for y in (False, True):
                f32("small", rows, F, y)
    for rows, F in BIG_CASES:
        for y in (False, True):
            f32("big", rows, F, y)
    for base in RAGGED_BASE:
        for w in RAGGED_W:
            f32("ragged", RAGGED_ROWS, base + w, False)
        for w in RAGGED_W_Y:
            f32("ragged", RAGGED_ROWS, base + w, True)
    for F, env in MAP_CASES:
        f32("map", MAP_ROWS, F, False, env)
    for F in KSPLIT_F:
        f32("ksplit", KSPLIT_ROWS, F, True)
    for F in F64_F:
        out.append(("f64(%d)" % F, f64_route(F, {})))
    for rows, F in SPLIT_DENSE:
        out.append(("split%s" % ((rows, F),), b16_route(F, {})))
    return out


# ---- exact data ---------------------------------------------------------------------------------------------------------
def _check_f32_exact(Phi, y):
    """No f32 accumulator of a K-split of <= 32 768 rows can leave the integers below 2^24 (module docstring)."""
    for r0 in range(0, Phi.shape[0], 32768):
        P = Phi[r0:r0 + 2 * 32768].astype(np.float64)
        s = (P * P).sum(axis=0).max()
        if y is not None:
            s = max(s, float((y[r0:r0 + 2 * 32768] ** 2).sum()))
        assert s < EXACT, (r0, s)


def _case(rows, F):
    """(Phi float32 in [-3, 3], y float64 in [-2, 2], G, b, yty in float64) -- computed once, shared, read-only (the two
    cases of hundreds of megabytes in a cache of their own, so that the many small ones do not push them out)."""
    return (_big_case if rows > 50000 else _small_case)(rows, F)


def _make_case(rows, F):
    rs = np.random.RandomState(rows * 7919 + F)
    Phi = rs.randint(-3, 4, size=(rows, F)).astype(np.float32)
    y = rs.randint(-2, 3, size=rows).astype(np.float64)
    _check_f32_exact(Phi, y)
    P = Phi.astype(np.float64)
    G, b, yty = P.T @ P, P.T @ y, float(y @ y)
    for a in (Phi, y, G, b):
        a.setflags(write=False)
    return Phi, y, G, b, yty


_big_case = functools.lru_cache(maxsize=2)(_make_case)
_small_case = functools.lru_cache(maxsize=3)(_make_case)


def _bf16_rne(x):
    """float32 -> bf16 (as float32), round to nearest even on the bits: bf16_rne of rr_syrk16.hip."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def _bf16_split(v):
    hi = _bf16_rne(v)
    return hi, _bf16_rne(v - hi)


def _split_values(rs, mask):
    h = np.where(mask, rs.choice([-2.0, -1.0, 1.0, 2.0], size=mask.shape), 0.0)
    l = np.where(mask, rs.choice([0.0, 2.0 ** -10, -2.0 ** -10], size=mask.shape), 0.0)
    v = (h + l).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), h + l)
    hi, lo = _bf16_split(v)
    assert np.array_equal(hi, h.astype(np.float32)) and np.array_equal(lo, l.astype(np.float32))
    return v, h, l


def _split_reference(h, l, y):
    hl = h.T @ l
    x3 = h.T @ h + hl + hl.T
    return x3, x3 + l.T @ l, None if y is None else (h + l).T @ y


def _check_split_exact(v, rps, bits):
    """Every partial sum of a K-split of `rps` rows (starting at a multiple of rps) is a multiple of 2^-bits below
    2^(24 - bits): the largest sum |v||v'| is a column's sum of squares."""
    a = v.astype(np.float64) ** 2
    for r0 in range(0, a.shape[0], rps):
        assert a[r0:r0 + rps].sum(axis=0).max() < 2.0 ** (24 - bits), (r0, rps, bits)


@functools.lru_cache(maxsize=2)
def _split_dense(rows, F):
    rs = np.random.RandomState(rows * 31 + F)
    v, h, l = _split_values(rs, rs.rand(rows, F) < 0.3)
    y = rs.randint(-2, 3, size=rows).astype(np.float64)
    return v, y, _split_reference(h, l, y)


@functools.lru_cache(maxsize=2)
def _split_sparse(rows, F):
    """At most three nonzeros per column in every aligned 64-row block."""
    rs = np.random.RandomState(rows * 37 + F)
    mask = np.zeros((_up(rows, 64), F), dtype=bool)
    nblk = mask.shape[0] // 64
    for k in range(3):
        r = rs.randint(0, 64, size=(nblk, F)) + 64 * np.arange(nblk)[:, None]
        mask[r, np.arange(F)[None, :]] = True
    v, h, l = _split_values(rs, mask[:rows])
    y = rs.randint(-2, 3, size=rows).astype(np.float64)
    _check_split_exact(v, 64, 20)
    return v, y, _split_reference(h, l, y)


@functools.lru_cache(maxsize=2)
def _split_sparse_long(rows, F):
    """At most one nonzero per column in every aligned 1100-row block: any K-split of up to 1087 rows, wherever it starts,
    spans two blocks and holds at most two nonzeros of a column (sum v^2 < 8.1 < 16, asserted over every window)."""
    rs = np.random.RandomState(rows * 41 + F)
    nblk = -(-rows // 1100)
    mask = np.zeros((nblk * 1100, F), dtype=bool)
    mask[rs.randint(0, 1100, size=(nblk, F)) + 1100 * np.arange(nblk)[:, None], np.arange(F)[None, :]] = True
    v, h, l = _split_values(rs, mask[:rows])
    cs = np.vstack([np.zeros((1, F)), np.cumsum(v.astype(np.float64) ** 2, axis=0)])
    w = min(1087, rows)
    assert (cs[w:] - cs[:-w]).max() < 16.0
    return v, _split_reference(h, l, None)


# ---- running a Gram -----------------------------------------------------------------------------------------------------
def _assert_bitwise(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d of %d differ, max |diff| %g" % (what, int(bad.sum()), bad.size, np.abs(got - want).max())


def _mismatch(got, want, what):
    """'' or a one-line description (the child processes collect these)."""
    try:
        _assert_bitwise(got, want, what)
    except AssertionError as e:
        return str(e)
    return ""


def _device():
    from revrand_amd import _hip
    return _hip.get_device()


class _Env(object):
    """Environment switches the launchers read per call, and deterministic mode, for the duration of a block."""

    def __init__(self, env=None, det=False, engine=None):
        self.env, self.det, self.engine = dict(env or {}), det, engine

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in PER_CALL}
        for k in PER_CALL:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in self.env.items() if v is not None})
        dev = _device()
        self.prev_engine = dev.set_gram_engine(self.engine) if self.engine else None
        self.prev_det = dev.set_deterministic(self.det)
        return self

    def __exit__(self, *exc):
        dev = _device()
        dev.set_deterministic(self.prev_det)
        if self.prev_engine:
            dev.set_gram_engine(self.prev_engine)
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Acc(object):
    """The device accumulators [G (F, F) | b (F) | yty] of gram_into, prefilled with K, kb, kt (default zeros)."""

    def __init__(self, F, K=None, kb=None, kt=0.0):
        from revrand_amd import _hip
        self.dev, self.F = _device(), F
        init = np.zeros(F * F + F + 1)
        if K is not None:
            init[:F * F] = np.asarray(K, dtype=np.float64).ravel()
        if kb is not None:
            init[F * F:F * F + F] = kb
        init[-1] = kt
        self.buf = self.dev.upload_vector(init)
        base = self.buf.ptr.value
        self.pG, self.pb, self.pt = (_hip.ctypes.c_void_p(base), _hip.ctypes.c_void_p(base + F * F * 8),
                                     _hip.ctypes.c_void_p(base + (F * F + F) * 8))

    def read(self, symmetrize):
        from revrand_amd import _hip
        F = self.F
        if symmetrize:
            _hip._check(self.dev.lib, self.dev.lib.rr_symmetrize_dev(self.dev.ctx, self.pG, F))
        out = self.dev.download(self.buf, (F * F + F + 1,), np.float64)
        return out[:F * F].reshape(F, F), out[F * F:F * F + F], float(out[-1])

    def free(self):
        self.buf.free()


def _gram(fm, Phi, y, acc, times=1, y_dtype=np.float32):
    """begin / put_host / gram_into (`times` times) of Phi's rows on feature matrix fm into the accumulators acc."""
    dev = _device()
    fm.begin(Phi.shape[0])
    fm.put_host(Phi, 0)
    dy = None if y is None else dev.upload_vector(y, dtype=y_dtype)
    for _ in range(times):
        if y is None:
            fm.gram_into(None, acc.pG)
        else:
            fm.gram_into(dy, acc.pG, acc.pb, acc.pt)
    dev.sync()
    if dy is not None:
        dy.free()


def run_gram(Phi, y=None, f64=False, env=None, det=False, engine=None):
    """(G, b, yty) of one Gram through a fresh FeatureMatrix / FeatureMatrix64 under the given switches, symmetrised."""
    from revrand_amd import _hip
    rows, F = Phi.shape
    fm = (_hip.FeatureMatrix64 if f64 else _hip.FeatureMatrix)(rows, F)
    acc = _Acc(F)
    try:
        with _Env(env, det, engine):
            _gram(fm, Phi, y, acc, y_dtype=np.float64 if f64 else np.float32)
        return acc.read(True)
    finally:
        acc.free()
        del fm


def _compare(got, want, what, with_y, last_block=None):
    """G, b, yty bit for bit; last_block = first column of the last 256-column block: reported on its own."""
    G, b, yty = got
    Gr, br, ytyr = want
    if last_block is not None:
        _assert_bitwise(G[:, last_block:], Gr[:, last_block:], what + ": last block's columns")
    _assert_bitwise(G, Gr, what + ": G")
    if with_y:
        _assert_bitwise(b, br, what + ": b")
        assert yty == ytyr, (what, yty, ytyr)


def _check_case(rows, F, with_y, env=None, det=False, last_block=None):
    Phi, y, G, b, yty = _case(rows, F)
    got = run_gram(Phi, y if with_y else None, env=env, det=det)
    _compare(got, (G, b, yty), "gram%s %s%s" % ((rows, F, with_y), env or "", " det" if det else ""), with_y, last_block)
    return got


# ---- tests: the route table ----------------------------------------------------------------------------------------------
def test_cases_cover_every_route():
    """The cases of this module, routed by the tables at this device's CU count, reach the small kernel, the main kernel
    alone (one column block), with the diagonal kernel, and with the ragged and the diagonal kernels; the tile map on and
    off -- with and without the diagonal kernel --, the rider and the gemv route for Phi^T y, both forms of the f64 pair, and
    the 16-bit launcher with and without its tile map."""
    cu = _device().compute_units
    hit = {}
    for label, r in route_cases(cu):
        keys = [route_name(r)]
        if r["kind"] == "main":
            keys.append("tile map %s, diagonal tiles %s" % ("on" if r["use_map"] else "off", "apart" if r["od"] else "in the main kernel"))
            if r["rg"]:
                keys.append("ragged kernel, w_last = %d%s" % (r["w_last"], " with the rider" if r["rider"] else ""))
        if r["engine"] == "f32":
            keys.append("%s, %s" % (r["kind"], "Phi^T y by the rider" if r["rider"] else
                                    "Phi^T y by the gemv kernel" if r["with_y"] else "no y"))
        if r["kind"] == "f64":
            keys = ["f64 nb = 1" if r["nb"] == 1 else "f64 nb >= 2"]
        if r["kind"] == "b16":
            keys = ["b16 tile map %s" % ("on" if r["use_map"] else "off")]
        for k in keys:
            hit.setdefault(k, label)
    for k in sorted(hit):
        print("%-52s %s" % (k, hit[k]))
    want = {"small", "main", "main+diag16", "main+ragged+diag16", "small, Phi^T y by the rider", "small, Phi^T y by the gemv kernel",
            "small, no y", "main, Phi^T y by the rider", "main, Phi^T y by the gemv kernel", "main, no y",
            "tile map on, diagonal tiles apart", "tile map off, diagonal tiles apart", "tile map on, diagonal tiles in the main kernel",
            "tile map off, diagonal tiles in the main kernel", "f64 nb = 1", "f64 nb >= 2", "b16 tile map on", "b16 tile map off"}
    want |= {"ragged kernel, w_last = %d" % w for w in RAGGED_W if w <= 192}
    want |= {"ragged kernel, w_last = %d with the rider" % (w + 1) for w in RAGGED_W_Y if w + 1 <= 192}
    assert want <= set(hit), sorted(want - set(hit))
    # 192 columns + the rider, and 193 columns, leave the ragged kernel
    assert not f32_route(RAGGED_ROWS, 1024 + 192, True, cu, {})["rg"] and not f32_route(RAGGED_ROWS, 1024 + 193, False, cu, {})["rg"]
    # the K-split cases reach the main kernel with and without the ragged kernel, besides the small one
    assert {route_name(f32_route(KSPLIT_ROWS, F, True, cu, {})) for F in KSPLIT_F} >= {"small", "main+ragged+diag16", "main+diag16"}
    # the child processes' cases: the A/B switches act on the main route, which RR_SYRK_SMALL=0 gives every width
    off = {"RR_SYRK_SMALL": "0"}
    assert {route_name(f32_route(r, F, takes_rider(F, y), cu, off)) for r, F, y in AB_CASES} == {"main", "main+diag16", "main+ragged+diag16"}
    assert {route_name(f32_route(r, F, takes_rider(F, y), cu, {})) for r, F, y in AB_CASES} >= {"small", "main+diag16", "main+ragged+diag16"}


def test_bf16_split_emulation():
    """The NumPy split used to build the 16-bit engines' data rounds to nearest even like bf16_rne (rr_syrk16.hip)."""
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, -2.0 - 2.0 ** -10, 1.0 - 2.0 ** -10, 0.0], dtype=np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -2.0, 1.0, 0.0], dtype=np.float32)
    assert np.array_equal(_bf16_rne(x), want)


# ---- tests: the f32 engine ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", SMALL_ROWS)
@pytest.mark.parametrize("F", SMALL_F)
def test_small_widths_are_exact(F, rows):
    """One to eight 128-column blocks of the small kernel, with the rider (a pad column) and by the gemv kernel (none)."""
    for with_y in (False, True):
        _check_case(rows, F, with_y)


@pytest.mark.parametrize("with_y", [False, True], ids=["G", "G,b"])
@pytest.mark.parametrize("rows,F", BIG_CASES)
def test_main_kernel_routes_are_exact(rows, F, with_y):
    """The main kernel alone on one column block, with the diagonal kernel at two and five blocks, and with the ragged one."""
    _check_case(rows, F, with_y, last_block=_up(F, 256) - 256)


@pytest.mark.parametrize("base", RAGGED_BASE)
@pytest.mark.parametrize("w,with_y", [(w, False) for w in RAGGED_W] + [(w, True) for w in RAGGED_W_Y])
def test_ragged_last_block_is_exact(w, with_y, base):
    """A last column block of w (+ 1 with the rider) live columns: zero to four live 32-column blocks per wave of the
    ragged kernel up to 192, the main and diagonal kernels above."""
    _check_case(RAGGED_ROWS, base + w, with_y, last_block=base)


@pytest.mark.parametrize("F,env", MAP_CASES, ids=lambda v: "+".join(sorted(v)) or "default" if isinstance(v, dict) else str(v))
def test_tile_map_routes_are_exact(F, env):
    """120 off-diagonal tiles (16 blocks; 17 with a ragged last one) and 136 / 120 tiles with the diagonal ones in the main
    kernel, through the XCD tile map and in plain order: one reference, and the same bits either way."""
    G, _, _ = _check_case(MAP_ROWS, F, False, env=env)
    if env.get("RR_GRAM_NO_TILE_MAP"):
        Gm, _, _ = _check_case(MAP_ROWS, F, False, env={})
        _assert_bitwise(G, Gm, "F = %d: without the tile map against with it" % F)


@pytest.mark.parametrize("rps", KSPLIT_RPS, ids=lambda v: "rps=%s" % v)
@pytest.mark.parametrize("F", KSPLIT_F)
def test_k_split_geometries_are_exact(F, rps):
    """125 k-blocks in splits of one, two and three k-blocks (a shorter last split), of 1024 rows, one split for all, and
    the launcher's own choice (the small kernel at F <= 768 ignores the variable)."""
    _check_case(KSPLIT_ROWS, F, True, env={"RR_GRAM_ROWS_PER_SPLIT": rps})


@pytest.mark.parametrize("rows,F,with_y", CONTRACT_CASES)
def test_gram_adds_to_the_upper_triangle_only(rows, F, with_y):
    """Into prefilled accumulators: upper triangle K + G, strict lower triangle still K (every flush is guarded by gr <= gc,
    the ragged kernel's transposed ones too), b and yty grown by Phi^T y and y^T y; a second call doubles the increments."""
    from revrand_amd import _hip
    Phi, y, G, b, yty = _case(rows, F)
    i, j = np.indices((F, F))
    K = ((3 * i + 5 * j) % 17 - 8).astype(np.float64)
    kb, kt = (np.arange(F) % 7 - 3).astype(np.float64), 11.0
    up = i <= j
    for times in (1, 2):
        fm, acc = _hip.FeatureMatrix(rows, F), _Acc(F, K, kb, kt)
        try:
            with _Env():
                _gram(fm, Phi, y if with_y else None, acc, times=times)
            Gd, bd, td = acc.read(False)
        finally:
            acc.free()
            del fm
        what = "gram%s x %d" % ((rows, F, with_y), times)
        _assert_bitwise(Gd[up], (K + times * G)[up], what + ": upper triangle")
        _assert_bitwise(Gd[~up], K[~up], what + ": strict lower triangle")
        _assert_bitwise(bd, kb + times * b if with_y else kb, what + ": b")
        assert td == (kt + times * yty if with_y else kt), (what, td)


@pytest.mark.parametrize("rows,F,with_y", DET_CASES)
def test_deterministic_mode_is_exact_and_repeats(rows, F, with_y):
    """The slabs and their ordered reduction (rr_syrk_det_reduce_kernel, one slab per K-split shared by the main, ragged
    and diagonal kernels) on one representative of every route: the exact result, twice."""
    first = _check_case(rows, F, with_y, det=True)
    again = _check_case(rows, F, with_y, det=True)
    _assert_bitwise(again[0], first[0], "repeat: G")
    _assert_bitwise(again[1], first[1], "repeat: b")


@pytest.mark.parametrize("F", REUSE_F)
def test_one_feature_matrix_through_changing_row_counts(F):
    """One FeatureMatrix at 1000 -> 37 -> 300 -> 1 -> 1000 rows, alternately with and without y: exact at every step, and
    after every call `download()` shows the pad columns (the rider's among them) of the live rows as zero.  The pad rows
    [rows, rows_pad) are not read back -- `download()` returns the live rows only; they, like the rows of a taller batch
    beyond them, are held by the next step's exact Gram alone, in which a stale row of integers would show."""
    from revrand_amd import _hip
    fm = _hip.FeatureMatrix(max(REUSE_ROWS), F)
    try:
        for step, rows in enumerate(REUSE_ROWS):
            with_y = step % 2 == 0
            Phi, y, G, b, yty = _case(rows + step, F)
            Phi, y = Phi[:rows], y[:rows]
            P = Phi.astype(np.float64)
            acc = _Acc(F)
            try:
                with _Env():
                    _gram(fm, Phi, y if with_y else None, acc)
                got = acc.read(True)
            finally:
                acc.free()
            _compare(got, (P.T @ P, P.T @ y, float(y @ y)), "step %d (%d rows, y %s)" % (step, rows, with_y), with_y)
            D = fm.download()
            _assert_bitwise(D[:, :F], Phi, "step %d: the feature columns" % step)
            _assert_bitwise(D[:, F:], np.zeros((rows, D.shape[1] - F), dtype=np.float32), "step %d: the pad columns" % step)
    finally:
        del fm


@pytest.mark.parametrize("rows,F", DENSE32_CASES)
def test_dense_gram_f32_is_exact(rows, F):
    """rr_dense_gram (rr_pack_f32_kernel, rr_gemv_t_kernel, the same launchers) on a view with ldphi > F, ragged rows."""
    from revrand_amd import _hip
    Phi, y, G, b, yty = _case(rows, F)
    wide = np.full((rows, F + 5), 7.0, dtype=np.float32)
    wide[:, :F] = Phi
    view = wide[:, :F]
    assert _hip._ld(_hip.as_float_matrix(view)) == F + 5
    with _Env():
        _compare(_hip.dense_gram(view, y), (G, b, yty), "dense_gram%s" % ((rows, F),), True, _up(F, 256) - 256)
        Gn, bn, tn = _hip.dense_gram(view)
    assert bn is None and tn is None
    _assert_bitwise(Gn, G, "dense_gram%s without y" % ((rows, F),))


# ---- tests: the f64 pair ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _case64(rows, F):
    rs = np.random.RandomState(rows * 104729 + F)
    Phi = rs.randint(-1000, 1001, size=(rows, F)).astype(np.float64)
    y = rs.randint(-1000, 1001, size=rows).astype(np.float64)
    assert max((Phi * Phi).sum(axis=0).max(), (y * y).sum()) < 2.0 ** 53
    return Phi, y, Phi.T @ Phi, Phi.T @ y, float(y @ y)


@pytest.mark.parametrize("F", F64_F)
def test_dense_gram_f64_is_exact(F):
    """float64 input keeps float64 arithmetic: products up to 10^6 that no f32 step would survive; one, two, three and nine
    128-column blocks (the off-diagonal kernel alone, then with the diagonal one), 1 to 5003 rows."""
    from revrand_amd import _hip
    for rows in F64_ROWS:
        Phi, y, G, b, yty = _case64(rows, F)
        with _Env():
            _compare(_hip.dense_gram(Phi, y), (G, b, yty), "dense_gram f64 %s" % ((rows, F),), True)


@pytest.mark.parametrize("F", F64_F)
def test_feature_matrix64_is_exact(F):
    """FeatureMatrix64 with y at the same widths and row counts; at 5003 rows into prefilled accumulators (upper triangle
    only), and in deterministic mode."""
    from revrand_amd import _hip
    for rows in F64_ROWS:
        Phi, y, G, b, yty = _case64(rows, F)
        _compare(run_gram(Phi, y, f64=True), (G, b, yty), "featmat64 %s" % ((rows, F),), True)
    _compare(run_gram(Phi, y, f64=True, det=True), (G, b, yty), "featmat64 %s det" % ((rows, F),), True)
    i, j = np.indices((F, F))
    K = ((i + 2 * j) % 13 - 6).astype(np.float64)
    kb, up = (np.arange(F) % 5).astype(np.float64), i <= j
    fm, acc = _hip.FeatureMatrix64(rows, F), _Acc(F, K, kb, 3.0)
    try:
        with _Env():
            _gram(fm, Phi, y, acc, times=2, y_dtype=np.float64)
        Gd, bd, td = acc.read(False)
    finally:
        acc.free()
        del fm
    _assert_bitwise(Gd[up], (K + 2 * G)[up], "featmat64 prefilled: upper triangle")
    _assert_bitwise(Gd[~up], K[~up], "featmat64 prefilled: strict lower triangle")
    _assert_bitwise(bd, kb + 2 * b, "featmat64 prefilled: b")
    assert td == 3.0 + 2 * yty


# ---- tests: the split 16-bit engines ------------------------------------------------------------------------------------
def _default_split_rows(rows, cu, F):
    """An upper bound of the rows per K-split rr_launch_syrk_bf16 picks by itself: 1024 (+ 63) while the row count is below
    1024 x unit (rr_launch_syrk_bf16's min_splits, unit, nsplit); asserted so that a case cannot slip outside the exactness argument."""
    from math import gcd
    nb = _up(F, 256) // 256
    unit = cu // gcd(cu, nb * (nb + 1) // 2)
    assert _up(rows, 64) < 1024 * unit, (rows, F, unit)
    return 1024 + 63


@pytest.mark.parametrize("rows,F", SPLIT_DENSE)
def test_split_engine_three_products_are_exact(rows, F):
    """bf16x3 on dense h + l data at the launcher's own K-splits: h^T h + h^T l + l^T h bit for bit (a dropped cross product
    or k-step, a swapped tile of the engine's own tile map at 15 and 16 blocks), Phi^T y by the gemv kernel; fp16x3, which
    falls back to the bf16x3 split on a host-put matrix, gives the same bits."""
    v, y, (x3, _, b) = _split_dense(rows, F)
    # multiples of 2^-10 below 2^14 over any K-split the launcher can pick here, whatever the density
    assert _default_split_rows(rows, _device().compute_units, F) * float(np.abs(v).max()) ** 2 < 2.0 ** 14
    G, bd, _ = run_gram(v, y, engine="bf16x3")
    _assert_bitwise(G, x3, "bf16x3 %s: G" % ((rows, F),))
    _assert_bitwise(bd, b, "bf16x3 %s: b" % ((rows, F),))
    if F <= 700:
        Gh, _, _ = run_gram(v, None, engine="fp16x3")
        _assert_bitwise(Gh, G, "fp16x3 %s against bf16x3" % ((rows, F),))
    if (rows, F) == (3001, 300):   # 47 splits of one 64-row pair of k-steps, the last holding one row
        G64, _, _ = run_gram(v, None, engine="bf16x3", env={"RR_GRAM_ROWS_PER_SPLIT": "64"})
        _assert_bitwise(G64, x3, "bf16x3 %s, 64-row splits: G" % ((rows, F),))


@pytest.mark.parametrize("rows,F", [(1000, 300), (3001, 700), (2016, 300), (1000, 4096)])
def test_split_engine_four_products_are_exact(rows, F):
    """bf16x4 on data with at most three nonzeros per column and 64-row block, in 64-row K-splits (module docstring): x3's
    sum + l^T l bit for bit; bf16x3 on the same data in 64-row splits and at its own."""
    v, y, (x3, x4, _) = _split_sparse(rows, F)
    assert (x4 != x3).any()
    rps = {"RR_GRAM_ROWS_PER_SPLIT": "64"}
    _assert_bitwise(run_gram(v, None, engine="bf16x4", env=rps)[0], x4, "bf16x4 %s" % ((rows, F),))
    _assert_bitwise(run_gram(v, None, engine="bf16x3", env=rps)[0], x3, "bf16x3 %s, 64-row splits" % ((rows, F),))
    _assert_bitwise(run_gram(v, None, engine="bf16x3")[0], x3, "bf16x3 %s" % ((rows, F),))
    # at the launcher's own K-splits (<= 1087 rows): one nonzero per column and 1100 rows, every k-step still holds some
    assert _default_split_rows(rows, _device().compute_units, F) <= 1087
    v, (x3, x4, _) = _split_sparse_long(rows, F)
    assert (x4 != x3).any()
    _assert_bitwise(run_gram(v, None, engine="bf16x4")[0], x4, "bf16x4 %s, the launcher's splits" % ((rows, F),))


# ---- the A/B variants, one child process each ---------------------------------------------------------------------------
def ab_child():
    """Run AB_CASES under this process' environment: the list of mismatches (empty when every result is exact)."""
    bad = []
    for rows, F, with_y in AB_CASES:
        Phi, y, G, b, yty = _case(rows, F)
        Gd, bd, td = run_gram(Phi, y if with_y else None)
        what = "gram%s" % ((rows, F, with_y),)
        bad += [m for m in (_mismatch(Gd, G, what + ": G"),) if m]
        if with_y:
            bad += [m for m in (_mismatch(bd, b, what + ": b"), "" if td == yty else what + ": yty") if m]
    return bad


def _child(code, env, timeout=600):
    code = ("import json, sys; sys.path[:0] = [%r, %r, %r]\nimport test_gpu_gram_exact as E\n" %
            (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))) + code
    e = {k: v for k, v in os.environ.items() if k not in AB_NAMES and k not in PER_CALL}
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)


_AB_STATE = {"failed": None}


def guarded_child(what, code, env, marker, timeout=600, forbidden=()):
    """Run `code` in a child process (`_child`) and return the JSON after its last `marker` line.  The children of this
    module and of the Gram census in tests/test_debug_builds.py run one after another and never on top of a failed one:
    a child that exits non-zero, prints no result, prints a `forbidden` word (a bounds report), runs into its time
    limit or is interrupted leaves `_AB_STATE` set, and every later call fails here without starting a process."""
    assert _AB_STATE["failed"] is None, "not started: the child for %s failed or hung" % (_AB_STATE["failed"],)
    _AB_STATE["failed"] = what            # until the child has shown otherwise, whatever ends this call
    try:
        r = _child(code, env, timeout)
    except subprocess.TimeoutExpired as e:   # killed and reaped by subprocess.run; nothing more runs on that card
        pytest.fail("the child for %s did not finish in %d s: %r %r" % (what, timeout, (e.stdout or "")[-1500:], (e.stderr or "")[-3000:]))
    lines = [l for l in r.stdout.splitlines() if l.startswith(marker + " ")]
    ok = r.returncode == 0 and lines and not any(w in r.stdout + r.stderr for w in forbidden)
    assert ok, (what, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    _AB_STATE["failed"] = None
    return json.loads(lines[-1][len(marker) + 1:])


@pytest.mark.parametrize("variant", AB_VARIANTS, ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()))
def test_ab_variants_are_exact(variant):
    """The kernels an environment variable switches in at process start -- no small kernel, the whole-block diagonal kernel,
    64-row k-blocks on the diagonal, the merged launch, the three earlier LDS-DMA forms of the main kernel, no split
    search -- give the same exact Gram.  One child process after another; none is started after one that failed, hung or
    was interrupted (`guarded_child`)."""
    assert guarded_child(variant, "print('ABRESULT', json.dumps(E.ab_child()))\n", variant, "ABRESULT") == []


# ---- which kernel ran (the bounds-checking build's launch counts; tests/test_debug_builds.py) ---------------------------
CENSUS_F32 = AB_CASES + [(37, 1, True), (1000, 256, True), (1000, 1024, False), (RAGGED_ROWS, 1024 + 192, True),
                         (RAGGED_ROWS, 1024 + 191, True), (RAGGED_ROWS, 512 + 64, False), (KSPLIT_ROWS, 1250, True)]
CENSUS_BIG = [(262149, 200, True), (87101, 500, False)]


def census(big=True):
    """Launches of each Gram kernel in one gram_into (or dense_gram) per case and mode, under a library that counts them
    (rr_debug_kernel_launches): [(label, compute units, {kernel: launches}, {kernel: launches the tables predict})]."""
    from revrand_amd import _hip
    dev = _device()
    lib, cu = dev.lib, dev.compute_units
    assert lib.rr_debug_kernel_launches(None) == 0
    out = []

    def one(label, Phi, y, route, f64=False, env=None, det=False, engine=None):
        rows, F = Phi.shape
        fm, acc = (_hip.FeatureMatrix64 if f64 else _hip.FeatureMatrix)(rows, F), _Acc(F)
        try:
            with _Env(env, det, engine):
                fm.begin(rows)
                fm.put_host(Phi, 0)
                dy = None if y is None else dev.upload_vector(y, dtype=np.float64 if f64 else np.float32)
                dev.sync()
                lib.rr_debug_kernel_launches(None)
                if y is None:
                    fm.gram_into(None, acc.pG)
                else:
                    fm.gram_into(dy, acc.pG, acc.pb, acc.pt)
                dev.sync()
                got = {k: int(lib.rr_debug_kernel_launches(k.encode())) for k in SYRK_KERNELS}
                e = dict(os.environ)
            want = predicted_launches(route(e), y is not None, det, e)
        finally:
            acc.free()
            del fm
        out.append((label, cu, got, want))

    for rows, F, with_y in CENSUS_F32 + (CENSUS_BIG if big else []):
        Phi, y = _case(rows, F)[:2]
        for det in (False, True):
            one("f32%s%s" % ((rows, F, with_y), " det" if det else ""), Phi, y if with_y else None,
                lambda e, a=(rows, F, with_y): f32_route(a[0], a[1], takes_rider(a[1], a[2]), cu, e), det=det)
    for F, env in MAP_CASES:
        Phi = _case(MAP_ROWS, F)[0]
        one("map%s" % ((MAP_ROWS, F, sorted(env)),), Phi, None, lambda e, F=F: f32_route(MAP_ROWS, F, False, cu, e), env=env)
    Phi, y = _case(KSPLIT_ROWS, 1100)[:2]
    for rps in ("32", "4096"):
        one("ksplit(1100, rps=%s)" % rps, Phi, y, lambda e: f32_route(KSPLIT_ROWS, 1100, True, cu, e), env={"RR_GRAM_ROWS_PER_SPLIT": rps})
    for F in F64_F:
        Phi, y = _case64(500, F)[:2]
        for det in (False, True):
            one("f64(500, %d)%s" % (F, " det" if det else ""), Phi, y, lambda e, F=F: f64_route(F, e), f64=True, det=det)
    for rows, F in [(1000, 300), (2016, 300), (1000, 4096)]:
        v, y = _split_sparse(rows, F)[:2]
        for engine in ("bf16x3", "bf16x4", "fp16x3"):
            one("%s%s" % (engine, (rows, F)), v, y, lambda e, F=F: b16_route(F, e), engine=engine)
    return out
