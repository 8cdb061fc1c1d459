"""Every route of the random Fourier feature kernels (rr_rff.hip) held element by element to derived bounds.

tests/rff_cases.py has the route table (`feature_route`), the two data families with their references and the bounds; this
module runs its cases through `_hip.RffHandle`, `lib.rr_rff_transform_dev`, `FeatureMatrix(64).put_rff` + `download` and
`gram_dev`:

* family A (dyadic phases of up to thousands of revolutions, exact in float32 in any summation order) leaves the sine /
  cosine instruction and the scale multiply as the only error: PHI_F32_BOUND per element, nothing for the phase;
* family B (real-valued data, at most two revolutions of sum |x Ws|) adds the forward bound of the projection;
* outputs of the device-resident calls are prefilled with a sentinel bit pattern: every element of the written block differs
  from it and meets its bound, every element outside still carries it, pad columns of a feature matrix are zero, and its pad
  rows [m, mpad), which `download` does not return, are shown zero by the matrix' own Gram;
* Phi^T y of the Gram's feature pass is held to the summed bounds, the feature-major second output to the transpose of P bit
  for bit (rr_featmat_download_pt; P^T holds the sentinel's transpose before the put, and keeps it outside the block), and
  identities that need no tolerance -- float32 and float64 inputs of the same values, a call split at a multiple of 32 rows,
  the three rescaling routes of the length scales -- are compared bit for bit;
* the switches read at process start (RR_FEATURES_NO_MFMA, RR_FEATURES_NO_MFMA64, RR_PREPARE_ON_HOST) run in child processes,
  one after another, none after one that failed (`guarded_child` of tests/test_gpu_gram_exact.py);
* `census` repeats the cases under the bounds-checking build and compares the launches per kernel with the route table
  (tests/test_debug_builds.py).  The launch counter drops template arguments: DMAX and the type pairs are held by the
  coverage test of tests/test_rff_cases_host.py and by the results alone.

A failure reports the route, the worst element's row, frequency and block, its phase and the ratio to its bound."""
import ctypes
import json
import os
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import rff_cases as R
from test_gpu_gram_exact import guarded_child

pytestmark = pytest.mark.gpu

CHILD_CODE = "import test_gpu_rff_exact as X\n"
CHILD_TIMEOUT = 420
_COUNT = {"on": False, "got": None}


def _hip():
    from revrand_amd import _hip
    return _hip


def _dev():
    return _hip().get_device()


class _Env(object):
    """A case's per-call environment (RR_FEAT_TPB is read at every launch); the process-start switches are the child's own."""

    def __init__(self, c):
        self.env = {k: v for k, v in c.env if k not in R.SWITCHES}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _measured(fn):
    """Run the one library call a case is about; under `census` count the kernels it launches."""
    if not _COUNT["on"]:
        return fn()
    dev = _dev()
    dev.sync()
    dev.lib.rr_debug_kernel_launches(None)
    out = fn()
    dev.sync()
    _COUNT["got"] = {k: int(dev.lib.rr_debug_kernel_launches(k.encode())) for k in R.FEATURE_KERNELS}
    return out


# ---- running a case -------------------------------------------------------------------------------------------------------------
def _upload_x(dev, h, c, D, xdt=None):
    """X in the padded layout.  ldx_extra: rows of dpad + extra elements, seen through a view one row into a taller matrix
    (stride and address off the 16-byte grid); ptr_off: a raw pointer that many bytes into a buffer."""
    T = R.NP[xdt or c.xdt]
    X = np.ascontiguousarray(D.X.astype(T))
    ld = h.padded_dim + c.ldx_extra
    if c.ptr_off:
        off = c.ptr_off // X.itemsize
        flat = np.zeros(c.rows * ld + off + 16, dtype=T)
        flat[off:off + c.rows * ld].reshape(c.rows, ld)[:, :c.d] = X
        buf = dev.upload_vector(flat)
        return SimpleNamespace(ptr=ctypes.c_void_p(buf.ptr.value + c.ptr_off), ld=ld, shape=X.shape, dtype=np.dtype(T), keep=buf)
    if c.ldx_extra:
        base = dev.upload_matrix(np.vstack([np.full((1, c.d), 7, dtype=T), X]), ld_dev=ld)
        return _hip().DeviceView(base, 1, c.rows)
    return dev.upload_matrix(X, ld_dev=h.padded_dim)


def _sentinel(dev, nelem, osz):
    return dev.upload_vector(np.full(nelem, R.SENTINEL[osz]))


def _check_block(label, raw, r0, r1, c0, c1):
    """raw: the whole buffer as unsigned integers.  Inside [r0, r1) x [c0, c1) nothing carries the sentinel, outside everything."""
    s = R.SENTINEL[raw.itemsize]
    inside = np.zeros(raw.shape, dtype=bool)
    inside[r0:r1, c0:c1] = True
    assert not np.any(raw[inside] == s), "%s: %d elements of the block were never written" % (label, int((raw[inside] == s).sum()))
    bad = np.argwhere((raw != s) & ~inside)
    assert bad.size == 0, "%s: %d elements outside the block were written, first at %s" % (label, len(bad), bad[:4].tolist())


def transform_dev(c, D, h, dX, row0=0, rows=None):
    """rr_rff_transform_dev of rows [row0, row0 + rows) into a sentinel-filled (rows + 2, 2n + 3) buffer: the written block."""
    hip, dev = _hip(), _dev()
    rows = c.rows - row0 if rows is None else rows
    T = R.NP[c.odt]
    osz, ldphi = np.dtype(T).itemsize, 2 * c.n + 3
    buf = _sentinel(dev, (rows + 2) * ldphi, osz)
    ls, lsp, nls = hip._lenscale_arg(R.lenscale_arg(D, c))
    xptr = ctypes.c_void_p(dX.ptr.value + row0 * dX.ld * np.dtype(dX.dtype).itemsize)
    with _Env(c):
        _measured(lambda: hip._check(dev.lib, dev.lib.rr_rff_transform_dev(h.h, xptr, hip.rr_dtype(dX.dtype), rows, dX.ld, lsp, nls, buf.ptr,
                                                                          hip.rr_dtype(T), ldphi)))
    dev.sync()
    raw = dev.download(buf, (rows + 2, ldphi), np.uint32 if osz == 4 else np.uint64)
    buf.free()
    _check_block(c.label, raw, 0, rows, 0, 2 * c.n)
    return np.ascontiguousarray(raw[:rows, :2 * c.n]).view(T)


def check_phi(c, D, got, route, amp=None, rows=slice(None), want=None, bound=None):
    arith = R.effective_arith(c.entry, c.compute)
    want = D.want[rows] if want is None else want
    assert got.shape == want.shape and got.dtype == R.NP[c.odt], (c.label, got.shape, want.shape, got.dtype)
    bound = R.phi_bound(arith, c.odt, c.family, c.d, D.A[rows], c.n) if bound is None else bound
    amp = np.sqrt(np.longdouble(c.n)) if amp is None else amp
    ratio, msg = R.report(c.label, route.rows, got.astype(np.longdouble) * amp, want, bound, D.phase[rows], c.n)
    print(msg)
    assert ratio <= 1.0, msg
    return ratio


def _check_gram(c, w, pb, G, amp2, u):
    """The upper triangle of G amp2 against w^T w.  The Gram itself is the SYRK suite's subject; here it shows that the pad rows
    [m, mpad) of the features hold zeros and nothing else: |d G_ij| <= sum_r (|w_ri| e_rj + |w_rj| e_ri + e_ri e_rj)
    + gamma(rows + 2) sum_r |w_ri w_rj|, e the per-element bounds and u the unit of the accumulation."""
    aw = np.abs(w)
    gb = aw.T @ pb + pb.T @ aw + pb.T @ pb + R.gamma(c.rows + 2, u) * (aw.T @ aw)
    iu = np.triu_indices(w.shape[1])
    gerr = np.abs(G * amp2 - w.T @ w)
    assert np.all(gerr[iu] <= gb[iu] + 1e-12), "%s: G is off by %.3f of its bound: pad rows of the features are not zero?" % (
        c.label, float((gerr[iu] / (gb[iu] + 1e-12)).max()))


def _pad_rows_are_zero(c, D, h, dX, f64):
    """Pad rows [m, mpad) of a feature matrix block (mpad = m rounded up to 16 in float64, to whole 32-row tiles in float32)
    are not part of `download`: seen through the matrix' own Gram.  The matrix first holds the sentinel in rows + 16 rows, so
    the rows behind the block are zero only if `begin` and the put left them so."""
    hip, dev = _hip(), _dev()
    T = np.float64 if f64 else np.float32
    F = 2 * c.n
    fm = (hip.FeatureMatrix64 if f64 else hip.FeatureMatrix)(c.rows + 16, F)
    fm.begin(c.rows + 16)
    fm.put_host(np.full((c.rows + 16, F), R.SENTINEL[np.dtype(T).itemsize]).view(T), 0)
    fm.begin(c.rows)
    fm.put_rff(h, dX, R.lenscale_arg(D, c), 0)
    dG = dev.zeros(F * F * 8)
    fm.gram_into(None, dG)
    dev.sync()
    G = dev.download(dG, (F, F), np.float64)
    dG.free()
    arith = R.effective_arith(c.entry, c.compute)
    pb = R.phi_bound(arith, c.odt, c.family, c.d, D.A, c.n)
    _check_gram(c, D.want.astype(np.float64), pb, G, float(c.n), R.U64 if f64 else R.U32)


def _gram(c, D, h, dX, route):
    hip, dev = _hip(), _dev()
    F, n = 2 * c.n, c.n
    acc = dev.zeros((F * F + F + 1) * 8)
    base = acc.ptr.value
    dy = dev.upload_vector(D.y.astype(R.NP[c.xdt])) if c.with_y else None
    args = (ctypes.c_void_p(base + F * F * 8), ctypes.c_void_p(base + (F * F + F) * 8)) if c.with_y else (None, None)
    prev = dev.set_deterministic(True) if c.det else None
    try:
        with _Env(c):
            _measured(lambda: h.gram_dev(dX, dy, R.lenscale_arg(D, c), ctypes.c_void_p(base), *args))
        dev.sync()
    finally:
        if c.det:
            dev.set_deterministic(prev)
    out = dev.download(acc, (F * F + F + 1,), np.float64)
    acc.free()
    G, b, yty = out[:F * F].reshape(F, F), out[F * F:F * F + F], out[-1]
    arith = R.effective_arith(c.entry, c.compute)
    pb = R.phi_bound(arith, "f32" if arith != "f64" else "f64", c.family, c.d, D.A, n)
    w = D.want.astype(np.float64)
    amp = np.sqrt(np.longdouble(n))
    if c.with_y:
        want_b = (D.y[:, None].astype(np.longdouble) * D.want).sum(axis=0)
        bb = R.bty_bound(arith, pb, D.want, D.y, c.rows)
        err = np.abs(b.astype(np.longdouble) * amp - want_b).astype(np.float64)
        f = int(np.argmax(err / bb))
        msg = "%s [%s]: Phi^T y worst at column %d: |error| %.3e, bound %.3e, ratio %.3f" % (c.label, "+".join(sorted(set(route.rows))), f,
                                                                                             err[f], bb[f], err[f] / bb[f])
        print(msg)
        assert np.all(err <= bb), msg
        assert yty == float((D.y ** 2).sum())
    _check_gram(c, w, pb, G, float(n), R.U64 if c.compute == "f64" else R.U32)
    assert not np.any(G[np.tril_indices(F, -1)]), c.label


def _featmat(c, D, h, dX, route):
    """put_rff / put_rff64 / put_gm at column 3 of a matrix of 5 more columns, prefilled with the sentinel through put_host.  The
    feature-major case (want_pt): a second pass over that sentinel matrix lays out P^T for this row count first, so P^T holds
    the sentinel's transpose when the measured put writes its block of it."""
    hip, dev = _hip(), _dev()
    f64 = c.entry == "put_rff64"
    T = np.float64 if f64 else np.float32
    width = (4 if c.entry == "put_gm" else 2) * c.n
    col0, F = 3, width + 5
    fm = (hip.FeatureMatrix64 if f64 else hip.FeatureMatrix)(c.rows, F)
    ls = R.lenscale_arg(D, c)
    fm.begin(c.rows)
    fm.put_host(np.full((c.rows, F), R.SENTINEL[np.dtype(T).itemsize]).view(T), 0)
    if c.want_pt:   # one transposing pass at this row count, over the sentinel
        dy = dev.upload_vector(D.y.astype(np.float32))
        fm.pass2_begin(np.ones(F) / F, np.eye(F))
        fm.pass2_rows(dy)
        fm.pass2_end()
    fm.begin(c.rows)
    with _Env(c):
        if c.entry == "put_gm":
            _measured(lambda: fm.put_gm(h, dX, np.zeros(c.d), np.broadcast_to(D.ls, (c.d,)).copy(), col0))
        else:
            _measured(lambda: fm.put_rff(h, dX, ls, col0))
    dev.sync()
    P = fm.download()
    raw = P.view(np.uint64 if f64 else np.uint32)
    _check_block(c.label, raw[:, :F], 0, c.rows, col0, col0 + width)
    assert not np.any(raw[:, F:]), "%s: pad columns are not zero" % c.label
    blk = np.ascontiguousarray(P[:, col0:col0 + width])
    if c.entry == "put_gm":   # a zero mean: two identical halves at amplitude sqrt(2 n)
        assert np.array_equal(blk[:, :2 * c.n], blk[:, 2 * c.n:])
        check_phi(c, D, np.ascontiguousarray(blk[:, :2 * c.n]), route, amp=np.sqrt(np.longdouble(2 * c.n)))
    else:
        check_phi(c, D, blk, route)
    if c.want_pt:
        Pt = fm.download_pt().view(np.uint32)
        r32 = (c.rows + 31) // 32 * 32
        _check_block(c.label + "/P^T", Pt[:F, :c.rows], col0, col0 + width, 0, c.rows)
        assert np.array_equal(Pt[col0:col0 + width, :c.rows], np.ascontiguousarray(blk.T).view(np.uint32)), \
            "%s: the feature-major output is not the transpose of P bit for bit" % c.label
        assert not np.any(Pt[col0:col0 + width, c.rows:r32]), "%s: pad rows of P^T are not zero" % c.label
    elif c.entry != "put_gm":
        _pad_rows_are_zero(c, D, h, dX, f64)


def _grad(c, D, h, route):
    arith = R.effective_arith(c.entry, c.compute)
    X = np.ascontiguousarray(D.X.astype(R.NP[c.xdt]))
    with _Env(c):
        got = _measured(lambda: h.grad(X, R.lenscale_arg(D, c), out_dtype=R.NP[c.odt]))
    want, adz = R.grad_reference(D, c)
    got = got.reshape(want.shape)
    bound = R.grad_bound(arith, c.odt, c.family, c.d, D.A, adz, c.d > 128)
    ratio, msg = R.report(c.label, route.rows, got.astype(np.longdouble) * np.sqrt(np.longdouble(c.n)), want, bound, D.phase, c.n)
    print(msg)
    assert ratio <= 1.0, msg
    # where x_i is zero the entry is zero whatever the phase: both blocks are compared, a dropped term shows in one of them
    assert not np.any(got[np.broadcast_to(adz == 0, got.shape)])


def _gm(c, D, h, route):
    arith = R.effective_arith(c.entry, c.compute)
    X = np.ascontiguousarray(D.X.astype(R.NP[c.xdt]))
    ls = R.lenscale_arg(D, c)
    amp = np.sqrt(np.longdouble(2 * c.n))
    ph4 = np.tile(D.phase, (1, 2))
    if c.entry == "gm_transform":
        got = _measured(lambda: h.gm_transform(X, D.mean, ls, out_dtype=R.NP[c.odt]))
        bound = R.gm_phi_bound(arith, c.odt, c.family, c.d, D.Agm, c.n)
        ratio, msg = R.report(c.label, route.rows, got.astype(np.longdouble) * amp, D.want4, bound, ph4, 2 * c.n)
        print(msg)
        assert ratio <= 1.0, msg
        return
    dm, dl = _measured(lambda: h.gm_grad(X, D.mean, ls, out_dtype=R.NP[c.odt]))
    wm, ax, wl, adz = R.gm_grad_reference(D, c)
    for name, got, want, mag, k in (("dmean", dm, wm, ax, R.GM_DMEAN_ROUNDINGS[arith]), ("dlen", dl, wl, adz, R.GRAD_ROUNDINGS[(arith, False)])):
        bound = R.gm_grad_bound(arith, c.odt, c.family, c.d, D.Agm, mag, k)
        ratio, msg = R.report(c.label + "/" + name, route.rows, got.reshape(want.shape).astype(np.longdouble) * amp, want, bound, ph4, 2 * c.n)
        print(msg)
        assert ratio <= 1.0, msg


def run_and_check(c):
    """One case: the call, its sentinel checks and its bounds.  Returns the route the table names for this device."""
    hip, dev = _hip(), _dev()
    route = R.case_route(c, dev.compute_units)
    assert route.error is None, (c.label, route.error)
    gm = c.entry in ("gm_transform", "gm_grad")
    D = R.gm_data(c) if gm else R.case_data(c)
    h = hip.RffHandle(D.W, compute=c.compute)
    if gm:
        _gm(c, D, h, route)
    elif c.entry == "grad":
        _grad(c, D, h, route)
    elif c.entry == "transform":
        X = np.ascontiguousarray(D.X.astype(R.NP[c.xdt]))
        got = _measured(lambda: h.transform(X, R.lenscale_arg(D, c), out_dtype=R.NP[c.odt]))
        check_phi(c, D, got, route)
    else:
        dX = _upload_x(dev, h, c, D)
        if c.entry == "transform_dev":
            check_phi(c, D, transform_dev(c, D, h, dX), route)
        elif c.entry == "gram":
            _gram(c, D, h, dX, route)
        else:
            _featmat(c, D, h, dX, route)
        getattr(dX, "base", getattr(dX, "keep", dX)).free()
    return route


def _ids(cases):
    return [c.label for c in cases]


# ---- tests ------------------------------------------------------------------------------------------------------------------
TRANSFORM, ALIGN, GRAD, LARGE = R.transform_cases(), R.align_cases(), R.grad_cases(), R.large_cases()
GRAM, FEATMAT, GM, HOST = R.gram_cases(), R.featmat_cases(), R.gm_cases(), R.host_cases()


@pytest.mark.parametrize("c", TRANSFORM, ids=_ids(TRANSFORM))
def test_transform_on_every_route_and_edge(c):
    """rr_rff_transform_dev: rows 1 .. 63 around both tile sizes, ragged 16-, 32- and 256-frequency blocks, Xdim 1 .. 128 in both
    families, every (x, out) type on every DMAX of the three arithmetics, the tiles-per-workgroup walk -- body on the matrix
    cores, remaining rows on the VALU kernel of the same call, into a sentinel-filled buffer."""
    run_and_check(c)


@pytest.mark.parametrize("c", ALIGN, ids=_ids(ALIGN))
def test_misaligned_rows_meet_the_bound(c):
    """A row stride or an address off the 16-byte grid (a view one row into a matrix of dpad + 1 columns; a raw pointer 8 bytes
    into a buffer) meets the same bounds.  The table sends the whole call to the VALU kernels (asserted of the table here);
    that it went there is seen by the census under the bounds-checking build alone."""
    r = run_and_check(c)
    assert not r.kernels["rr_rff_features_mfma_kernel"] and not r.kernels["rr_rff_features_mfma64_kernel"]


@pytest.mark.parametrize("c", GRAD, ids=_ids(GRAD))
def test_grad_entries_relative_to_their_own_dz(c):
    """dPhi / dl_i, each entry against its own |dz_i| / sqrt(n): both blocks, every dimension of ARD length scales, dimension 0
    alone for an isotropic one (the reference's quirk), exact zeros where x_i is zero."""
    run_and_check(c)


@pytest.mark.parametrize("c", LARGE, ids=_ids(LARGE))
def test_large_xdim_routes(c):
    """Xdim 129 and 200: GEMM with the cos / sin epilogue, GEMM + rr_trig_kernel, rr_phase_f64_kernel + rr_trig_kernel through
    transform, grad, the Gram's feature pass and both feature matrices; RR_LG_ROWS + 1 rows cross the sub-chunk seam."""
    run_and_check(c)


@pytest.mark.parametrize("c", GRAM, ids=_ids(GRAM))
def test_gram_feature_pass_and_its_targets(c):
    """Phi^T y from the feature pass (HAS_Y; atomics and deterministic mode) against sum_r y_r Phi_rf, integer y in [-3, 3]; the
    upper triangle of G shows zero pad rows; y^T y is exact."""
    run_and_check(c)


@pytest.mark.parametrize("c", FEATMAT, ids=_ids(FEATMAT))
def test_feature_matrix_blocks(c):
    """FeatureMatrix / FeatureMatrix64 blocks at a column offset: the block meets its bound, the other columns keep the
    sentinel, pad columns are zero; with a P^T laid out, the feature-major second output is the transpose of P bit for bit."""
    run_and_check(c)


@pytest.mark.parametrize("c", GM, ids=_ids(GM))
def test_spectral_mixture_kernels(c):
    """rr_gm_transform_kernel / rr_gm_grad_kernel: phases z +- x . mean / (2 pi) in both families."""
    run_and_check(c)


@pytest.mark.parametrize("c", HOST, ids=_ids(HOST))
def test_host_entry_points(c):
    run_and_check(c)


def test_grid_clamp_of_the_matrix_core_kernel():
    """RR_FEAT_TPB=1 with 32 * 65536 + 32 rows: 65537 row tiles, two per workgroup after the clamp; every row is written."""
    r = run_and_check(R.CLAMP_MFMA)
    assert r.grids[0][1:] == (1, 32769, 2)


def _bits(c, xdt=None, split=None):
    hip, dev = _hip(), _dev()
    D = R.case_data(c)
    h = hip.RffHandle(D.W, compute=c.compute)
    dX = _upload_x(dev, h, c, D, xdt)
    if split is None:
        return transform_dev(c, D, h, dX)
    return np.vstack([transform_dev(c, D, h, dX, 0, split), transform_dev(c, D, h, dX, split, c.rows - split)])


IDENT = [R.case("id/%s/d=%d" % (cp, d), "transform_dev", cp, 32 * 5 + 21, d, 70, family="B", seed=d, ard=True, xdt="f32", odt=odt)
         for cp, odt in (("f32", "f32"), ("f64", "f64")) for d in (9, 100)]


@pytest.mark.parametrize("c", IDENT, ids=_ids(IDENT))
def test_identities_that_need_no_tolerance(c):
    """The same kernel on the same values: float32 and float64 inputs of float32-representable data, and a call split at a
    multiple of 32 rows, give the bits of the whole."""
    whole = _bits(c)
    U = np.uint32 if c.odt == "f32" else np.uint64
    assert np.array_equal(whole.view(U), _bits(c, xdt="f64").view(U)), "float64 input of the same values"
    assert np.array_equal(whole.view(U), _bits(c, split=64).view(U)), "split at 64 rows"
    assert np.array_equal(whole.view(U), _bits(c, split=160).view(U)), "split at 160 rows"


def prepare_bits():
    """Family A through the table rr_basis_prepare wrote in this process: CRC of Phi (64 frequencies: 1 / sqrt(n) = 1/8)."""
    c = R.PREPARE_IDENTITY
    return int(zlib.crc32(_bits(c).tobytes()))


def test_prepare_routes_write_the_same_table():
    """rr_scale_w_kernel (here), host scaling (the RR_PREPARE_ON_HOST child compares its CRC with this one) and
    rr_basis_prepare_dev give identical Phi bits on family A.  The device-side route scales a spectral-mixture block by
    1 / sqrt(2 n): at n = 32 that is 1/8 like 1 / sqrt(64), so a zero-mean put_gm of the first 32 frequencies is compared bit
    for bit with those columns of the 64-frequency transform."""
    hip, dev = _hip(), _dev()
    c = R.PREPARE_IDENTITY
    D = R.case_data(c)
    whole = _bits(c)
    n2 = c.n // 2
    h = hip.RffHandle(D.W[:, :n2].copy(), compute="f32")
    dX = _upload_x(dev, h, c, D)
    fm = hip.FeatureMatrix(c.rows, 4 * n2)
    fm.begin(c.rows)
    fm.put_gm(h, dX, np.zeros(c.d), np.broadcast_to(D.ls, (c.d,)).copy(), 0)
    P = fm.download()[:, :4 * n2]
    for blk in (0, 2 * n2):
        assert np.array_equal(P[:, blk:blk + n2].view(np.uint32), whole[:, :n2].view(np.uint32)), "cos block at %d" % blk
        assert np.array_equal(P[:, blk + n2:blk + 2 * n2].view(np.uint32), whole[:, c.n:c.n + n2].view(np.uint32)), "sin block at %d" % blk


def test_a_float64_phase_basis_refuses_misaligned_rows():
    """No VALU kernel takes the float32 sine / cosine of a float64 phase: the Gram and the feature matrix say so."""
    hip, dev = _hip(), _dev()
    c = R.case("refuse", "gram", "f32p64", 70, 9, 33, ldx_extra=1)
    assert R.case_route(c, dev.compute_units).error
    D = R.case_data(c)
    h = hip.RffHandle(D.W, compute="f32p64")
    dX = _upload_x(dev, h, c, D)
    G = dev.zeros(66 * 66 * 8)
    with pytest.raises(hip.HipError, match="16-byte aligned"):
        h.gram_dev(dX, None, 1.0, G)
    fm = hip.FeatureMatrix(70, 66)
    fm.begin(70)
    with pytest.raises(hip.HipError, match="16-byte aligned"):
        fm.put_rff(h, dX, 1.0, 0)
    dev.sync()


def switch_child(switch, want_crc=None):
    """Entry point of a child started with one process-start switch: its cases, and the CRC of the prepare identity."""
    assert os.environ.get(switch) is not None
    bad = []
    for c in R.switch_cases(switch):
        try:
            run_and_check(c)
        except AssertionError as e:
            bad.append((c.label, str(e)[:600]))
    if switch == "RR_PREPARE_ON_HOST" and prepare_bits() != want_crc:
        bad.append(("prepare identity", "host scaling and rr_scale_w_kernel give different Phi bits"))
    return bad


@pytest.mark.parametrize("switch", R.SWITCHES)
def test_switches_read_at_process_start(switch):
    """RR_FEATURES_NO_MFMA (the VALU kernels at every DMAX, Phi^T y plain and deterministic, the grid clamp of grad at
    16 * 65535 + 17 rows and transform at that size), RR_FEATURES_NO_MFMA64 (the LDS-staged float64 kernels) and
    RR_PREPARE_ON_HOST (host scaling: same bits as the kernel's table), each in a child process, one after another, none after
    one that failed or hung."""
    crc = prepare_bits() if switch == "RR_PREPARE_ON_HOST" else None
    got = guarded_child("the feature kernels under %s" % switch, CHILD_CODE + "print('RFFRESULT', json.dumps(X.switch_child(%r, %r)))\n"
                        % (switch, crc), {switch: "1"}, "RFFRESULT", timeout=CHILD_TIMEOUT, forbidden=("RR_BOUNDS",))
    assert got == [], got


# ---- which kernel ran (the bounds-checking build's launch counts; tests/test_debug_builds.py) --------------------------------
def census(switch=None):
    """One call per census case under a library that counts launches (rr_debug_kernel_launches): [(label, compute units,
    {kernel: launches}, {kernel: launches the table predicts}, failure of the case's own checks or None)]."""
    dev = _dev()
    assert dev.lib.rr_debug_kernel_launches(None) == 0
    cases = R.census_cases() if switch is None else [c for c in R.switch_cases(switch) if not c.big]
    out = []
    _COUNT["on"] = True
    try:
        for c in cases:
            _COUNT["got"], wrong = None, None
            try:
                route = run_and_check(c)
            except AssertionError as e:
                wrong, route = str(e)[:400], R.case_route(c, dev.compute_units)
            out.append((c.label, dev.compute_units, _COUNT["got"], route.counts(), wrong))
    finally:
        _COUNT["on"] = False
    return out
