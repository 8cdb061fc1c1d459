"""Every kernel route of the second data pass of `_elbo` and of predict_moments against exact references, bit for bit.

The drivers pick their kernels from the layout, the row count, the input dimension, the engine and the CU count:
rr_featmat_pass2_rows_planned / rr_featmat_pass2_rff / fm_pass2_products / rr_featmat_predict_rows for a feature matrix,
pass2_run for a single random Fourier basis, launch_gemm_gradt, launch_features_t and launch_grad_t below them
(rr_elbo.hip), and the float64 family (FeatureMatrix64).  `pass2_route`, `predict_route` and `basis_route` restate those
rules and return the launches they expect of the kernels in KERNELS; `test_cases_cover_every_route` asserts, at the CU
count of the device it runs on, that the cases below reach every row of the table in docs/KERNELS.md 3.5, and `census`
(tests/test_debug_builds.py) compares the launch counts of the bounds-checking build with the tables.  The launch
counter drops template arguments, so it cannot tell NXB = 1 | 2 | 4, DM = 8 .. 128 or rr_rows64_kernel<0 | 1> apart:
those are reached by the case lists (asserted by the coverage test) and held by the exact results alone.

Two data sets make every quantity exact whatever the summation order, the assignment of row tiles to workgroups, the
K-range of a tile or the atomics:

* Feature matrix (part 1).  The feature-matrix protocol contracts whatever sits in P: `put_host` writes any block, and
  pass2_plan_rff / pass2_rows_planned / pass2_rff take an RffHandle only for n, d and the padded layout of X.  Phi is
  ternary (15 % nonzero), m in {-2 .. 2} (nonzero with probability min(0.5, 6 / F)), C symmetric with ternary
  off-diagonals (about 6 per column) and diagonal in {1, 2}, B the upper triangle of such a matrix, X in {-2 .. 2}, y in
  {-3 .. 3}.  Then dot = Phi m, err = y - dot, sqErr, U = Phi C, A = err (Pc ms - Ps mc) - (Pc Us - Ps Uc), T = X^T A, Ey,
  Vf = rowsum((Phi Ctri) o Phi) and Vf = rowsum((Phi B)^2) are integers.  Float64: entries up to +-1000 in Phi and y,
  +-100 in X, +-10 in m and C; every sum of absolute values asserted below 2^53, most far above 2^24.
* Quarter turns (part 2, `RffHandle.elbo_pass2` / `.predict`, and one `put_rff` child of part 1).  lenscale = 1,
  W = (pi / 2) Q with Q integer in [-3, 3], X ternary (5 - 10 % nonzero): float32(W / 2 pi) == Q / 4 (asserted), every phase
  is a multiple of a quarter revolution, and with n a power of four 1 / sqrt(n) is a power of two: every feature is 0 or
  +-1 / sqrt(n) -- IF v_sin_f32 / v_cos_f32 are exact there, which `test_quarter_turn_features_are_exact` asserts first
  (through RffHandle.transform and FeatureMatrix.put_rff + download; docs/KERNELS.md 3.5 records the outcome).  Everything
  downstream is then a multiple of s = 1 / sqrt(n) (dot, err, U) or of s^2 (A, T, sqErr, Vf).

Conditions asserted on the host per case, before any comparison, in units of those quanta (`_reference`,
`_predict_reference`): max_r ||Phi_r||_1 max(|C|, |m|) < 2^24 (every entry of U and of dot, any order); |err| < 2^24;
max_{i,f} sum_r |X_ri| (|err_r| (|Pc| |ms| + |Ps| |mc|) + |Pc| |Us| + |Ps| |Uc|) < 2^24 over ALL rows of the case (any tiling);
sum_c U_rc^2 < 2^24 (the rowsq epilogue) and sum_c |U_rc| |Phi_rc| < 2^24 (rr_rowdot_kernel); every reference Vf is
nonzero; at least 95 % of the reference's T is nonzero from 1000 rows on.  Below that no data of this kind can promise it:
an entry of T is a sum of about 0.8 x 0.2 x rows small random integers (X is zero in 20 % of its entries, A in about
80 %) and such a sum is zero with probability about 1 / (sigma sqrt(2 pi)) -- 5 - 6 % at 256 rows, and at one row T = x A^T
carries the zeros of both factors -- so those cases assert 90 % from 256 rows on and a nonzero T below; dT is prefilled with
nonzero integers everywhere and T is accumulated into it, so `==` is never vacuous.  The references themselves are float32 / float64 NumPy
products of the same integers, exact under the same bounds.
"""
import functools
import os

import numpy as np
import pytest

from test_gpu_gram_exact import guarded_child

pytestmark = pytest.mark.gpu

EXACT = 1 << 24
KERNELS = ["rr_gemm_gradt_f32_kernel", "rr_gemm_tn_f32_kernel", "rr_gemm_pair_f32_kernel", "rr_grad_t_kernel", "rr_err_kernel",
           "rr_rowdot_kernel", "rr_rowvec_kernel", "rr_transpose_f32_kernel", "rr_rff_features_t_kernel",
           "rr_rff_features_t4_kernel", "rr_c64_to_c32_kernel", "rr_split_bf16_kernel", "rr_syrk_b16w4_kernel",
           "rr_transpose_f64_kernel", "rr_rows64_kernel", "rr_err64_kernel", "rr_grad_t64_kernel"]
# read per call (getenv in the drivers / in GemmArgs' initialiser); RR_PREDICT_NO_FUSE per call by rr_featmat_predict_rows only
PER_CALL = ("RR_PASS2_NO_FUSE", "RR_PREDICT_NO_FUSE", "RR_PREDICT_NO_DIAG_SKIP", "RR_PASS2_CHUNK_ROWS")
# read once per process (static const): fm_pass2_products and pass2_run, launch_features_t, pass2_run
STATICS = [{"RR_PREDICT_NO_PAIR": "1"}, {"RR_FEATURES_T_NO_SPLIT": "1"}, {"RR_PREDICT_NO_FUSE": "1"}]
STATIC_NAMES = sorted({k for v in STATICS for k in v})


# ---- the route tables ---------------------------------------------------------------------------------------------------
def _up(n, m):
    return (n + m - 1) // m * m


def _on(env, name):
    """`const char *v = getenv(name); v && atoi(v) != 0`."""
    v = env.get(name)
    try:
        return v is not None and int(v) != 0
    except ValueError:
        return False


def _dm(d):
    """rr_pick_dmax: the DM instance of rr_grad_t_kernel / the feature-major kernels (0: Xdim > 128, no instance)."""
    return next((p for p in (8, 16, 32, 64, 128) if d <= p), 0)


def gradt_geometry(rows, n, d, cu):
    """launch_gemm_gradt: NXB, column tiles, row tiles, workgroups per column tile and the row tiles each one walks."""
    ntb, nta = 2 * n // 256, _up(rows, 256) // 256
    G = min(max(cu // ntb, 1), nta)
    nxb = (d + 31) // 32
    return {"nxb": 1 if nxb <= 1 else 2 if nxb == 2 else 4, "ntb": ntb, "nta": nta, "G": G, "walk": -(-nta // G),
            "partial": rows % 256 != 0}


def pass2_route(rows, F, children, cu, engine="f32", det=False, env=None, x64=False, pt_covered=False, cb_ready=False):
    """rr_featmat_pass2_begin (host C) .. rr_featmat_pass2_rows_planned .. rr_featmat_pass2_rff of every child (col0, n, d):
    whether the planned children are contracted inside the product, and {kernel: launches}."""
    env = os.environ if env is None else env
    fused = (bool(children) and engine == "f32" and not det and not _on(env, "RR_PASS2_NO_FUSE") and not x64 and
             all(col0 % 256 == 0 and n % 256 == 0 and d <= 128 for col0, n, d in children))     # `ok`
    k = dict.fromkeys(KERNELS, 0)
    k["rr_rowvec_kernel"] = k["rr_err_kernel"] = 1
    k["rr_transpose_f32_kernel"] = 0 if pt_covered else 1
    r = {"fused": fused, "kernels": k, "K": _up(F, 32), "live_last_kblock": F - (_up(F, 32) - 32), "ld": _up(F, 256)}
    if fused:
        k["rr_gemm_gradt_f32_kernel"] = len(children)
        r["gradt"] = [gradt_geometry(rows, n, d, cu) for col0, n, d in children]
        return r
    if engine == "f32":
        k["rr_gemm_tn_f32_kernel"] = 1               # fm_pass2_products: never the pair kernel (upper_b = 0)
    else:
        k["rr_split_bf16_kernel"], k["rr_syrk_b16w4_kernel"] = 1 if cb_ready else 2, 1
    k["rr_grad_t_kernel"] = sum(-(-d // 128) if d > 128 else 1 for col0, n, d in children)      # launch_grad_t
    r["dm"] = [_dm(d) for col0, n, d in children]
    return r


def predict_route(rows, F, form, cu, engine="f32", det=False, env=None, c_dev=False, cb_ready=False):
    """rr_featmat_predict_begin[_b] .. rr_featmat_predict_rows.  form 0: C in triangular form (host, or c_dev: converted
    by rr_c64_to_c32_kernel), Vf = rowdot(U, P); form 1: the caller's factor B, Vf summed in the product's epilogue or
    (split engine, deterministic mode, RR_PREDICT_NO_FUSE) by rr_rowdot_kernel(U, U)."""
    env = os.environ if env is None else env
    ntb = _up(F, 256) // 256
    fused_vf = form == 1 and engine == "f32" and not det and env.get("RR_PREDICT_NO_FUSE") is None
    pair = engine == "f32" and env.get("RR_PREDICT_NO_PAIR") is None
    k = dict.fromkeys(KERNELS, 0)
    k["rr_rowvec_kernel"] = k["rr_transpose_f32_kernel"] = 1
    k["rr_c64_to_c32_kernel"] = 1 if c_dev and form == 0 else 0
    if engine != "f32":
        k["rr_split_bf16_kernel"], k["rr_syrk_b16w4_kernel"] = 1 if cb_ready else 2, 1
    else:
        k["rr_gemm_pair_f32_kernel" if pair else "rr_gemm_tn_f32_kernel"] = 1
    k["rr_rowdot_kernel"] = 0 if fused_vf else 1
    return {"kernels": k, "ntb": ntb, "pair": pair, "fused_vf": fused_vf, "form": form,
            "diag_skip": pair and env.get("RR_PREDICT_NO_DIAG_SKIP") is None,
            "pairs": "one tile" if ntb == 1 else "even" if ntb % 2 == 0 else "odd"}


def f64_route(children, pred=False):
    """FeatureMatrix64 (fm64_products + rr_featmat64_pass2_rows / _pass2_rff / _predict_rows): one route, one kernel each."""
    k = dict.fromkeys(KERNELS, 0)
    k["rr_transpose_f64_kernel"] = k["rr_rows64_kernel"] = 1
    if not pred:
        k["rr_err64_kernel"], k["rr_grad_t64_kernel"] = 1, len(children)
    return {"kernels": k, "f64": "predict" if pred else "gradient"}


def basis_route(N, d, n, cu, pred=False, form=0, x64=False, compute="f32", det=False, env=None):
    """pass2_run for one random Fourier basis (rr_rff_elbo_pass2_dev, rr_rff_predict_dev / devb): the row chunks, how
    the feature-major operand is made, whether the gradient pass is fused, and {kernel: launches}."""
    env = os.environ if env is None else env
    Fp = _up(2 * n, 256)
    chunk = (24 << 30) // (12 * Fp)
    ce = env.get("RR_PASS2_CHUNK_ROWS")
    if ce and int(ce) >= 256:
        chunk = int(ce)
    elif N > chunk:
        chunk = -(-N // -(-N // chunk))
    chunk = _up(min(chunk, N), 256)
    chunks = [min(chunk, N - r0) for r0 in range(0, N, chunk)]
    large, phase64 = d > 128, compute == "f32p64"
    fuse_t = (not pred and not x64 and not det and not large and not phase64 and n % 256 == 0 and d <= 128 and
              not _on(env, "RR_PASS2_NO_FUSE"))
    fuse_vf = pred and form == 1 and not det and env.get("RR_PREDICT_NO_FUSE") is None          # will_fuse_vf
    k = dict.fromkeys(KERNELS, 0)
    feats = set()
    for mrows in chunks:
        mpad = _up(mrows, 256)
        if large or phase64:
            k["rr_transpose_f32_kernel"] += 1
            k["rr_rowvec_kernel"] += 1
            feats.add("transpose")
        else:
            few = env.get("RR_FEATURES_T_NO_SPLIT") is None and mpad // 256 < 2 * cu and n >= 16
            k["rr_rff_features_t4_kernel" if few else "rr_rff_features_t_kernel"] += 1
            feats.add("t4" if few else "t")
        if fuse_t:
            k["rr_err_kernel"] += 1
            k["rr_gemm_gradt_f32_kernel"] += 1
            continue
        k["rr_gemm_pair_f32_kernel" if pred and env.get("RR_PREDICT_NO_PAIR") is None else "rr_gemm_tn_f32_kernel"] += 1
        if pred:
            k["rr_rowdot_kernel"] += 0 if fuse_vf else 1
        else:
            k["rr_err_kernel"] += 1
            k["rr_grad_t_kernel"] += -(-d // 128) if large else 1
    k["rr_c64_to_c32_kernel"] = 0
    return {"fused": fuse_t, "kernels": k, "chunks": chunks, "features": feats, "fused_vf": fuse_vf,
            "need_p": not (fuse_vf and not large and not phase64), "dm": _dm(d),
            "gradt": [gradt_geometry(mrows, n, d, cu) for mrows in chunks] if fuse_t else []}


# ---- the cases ----------------------------------------------------------------------------------------------------------
# feature-matrix layouts: F and the planned children (col0, n); everything outside the children is a host ("linear") block
LAYOUTS = {"one": (512, [(0, 256)]),                        # one child, whole tiles
           "behind": (768, [(256, 256)]),                   # the same child behind a 256-column host block: B = C32 + col0
           "two+linear": (1027, [(0, 256), (512, 256)]),    # K = 1056, 3 live rows in the last k-block, U[:, 1024:] unneeded
           "n1024": (2048, [(0, 1024)]),
           "col3": (515, [(3, 256)]),                       # stored: the child is not tile aligned
           "n150": (300, [(0, 150)])}                       # stored: n is no multiple of 256
FUSED_LAYOUTS = ["one", "behind", "two+linear", "n1024"]
SWEEP_LAYOUTS = ["one", "behind", "two+linear", "col3", "n150"]     # x GRAD_ROWS; n1024 runs once, at 9000 rows
GRAD_ROWS = [1, 37, 256, 257, 1000, 5003]
GRAD_D = 8
BIG_GRAD = [("n1024", 9000, 40), ("one", 40000, 8)]        # G = 32 < nta = 36 and G = 128 < nta = 157 on 256 CUs
NXB_D = [5, 32, 33, 64, 65, 100, 128]                       # NXB 1, 1, 2, 2, 4, 4, 4; DM 8, 32, 64, 64, 128, 128, 128
DM_D = [5, 9, 32, 64, 100, 130]                             # DM 8, 16, 32, 64, 128 and Xdim > 128 (two launches)
NXB_ROWS = 1000
REUSE_ROWS = [1000, 37, 300]
DET_CASES = [("one", 1000, 8), ("col3", 1000, 8), ("n150", 5003, 20), ("two+linear", 257, 8)]
PRED_F = [200, 512, 700, 1000, 1100, 1280]                  # ntb = 1, 2, 3, 4, 5, 5
PRED_ROWS = [1, 37, 257, 1000]
PRED_MODES = ["form0 host", "form0 device", "form1 fused", "form1 stored", "form1 det", "form0 no diag skip", "form1 no diag skip"]
ENGINES = ["bf16x3", "bf16x4", "fp16x3"]
F64_F = [100, 130, 300]
F64_ROWS = [1, 17, 500]
F64_CHILD = {100: (0, 50, 5), 130: (2, 64, 20), 300: (44, 128, 70)}     # (col0, n, d)
# single basis, quarter turns: (rows, d, n)
QT_FUSED = [(3000, 5, 256), (1500, 32, 256), (2100, 33, 1024), (1500, 64, 256), (900, 100, 256)]
QT_CHUNKS = [None, "768", "256"]       # in this order on one handle: the scratch of the larger call serves the smaller ones
QT_STORED = [(700, 5, 16, {}), (700, 9, 64, {}), (700, 5, 256, {"x64": True}), (700, 5, 256, {"compute": "f32p64"}),
             (700, 130, 256, {}), (700, 5, 256, {"det": True}), (700, 20, 64, {"det": True})]
QT_BIG = (131328, 8, 256)              # 513 row tiles >= 2 x 256 CUs: the plain feature-major kernel
QT_PREDICT = [(257, 5, 256), (1000, 33, 1024), (700, 5, 64), (700, 130, 256)]


def route_cases(cu):
    """(label, route) of every call the tests below make under the default switches or the per-call ones."""
    out = []
    for name in SWEEP_LAYOUTS:
        F, kids = LAYOUTS[name]
        for rows in GRAD_ROWS:
            ch = [(c0, n, GRAD_D) for c0, n in kids]
            out.append(("grad %s x %d" % (name, rows), pass2_route(rows, F, ch, cu, env={})))
            out.append(("grad %s x %d stored" % (name, rows), pass2_route(rows, F, ch, cu, env={"RR_PASS2_NO_FUSE": "1"})))
    for name, rows, d in BIG_GRAD:
        F, kids = LAYOUTS[name]
        out.append(("grad %s x %d" % (name, rows), pass2_route(rows, F, [(c0, n, d) for c0, n in kids], cu, env={})))
    for d in NXB_D:
        out.append(("grad one x %d, d = %d" % (NXB_ROWS, d), pass2_route(NXB_ROWS, 512, [(0, 256, d)], cu, env={})))
    for d in DM_D:
        out.append(("grad one x %d, d = %d stored" % (NXB_ROWS, d),
                    pass2_route(NXB_ROWS, 512, [(0, 256, d)], cu, env={"RR_PASS2_NO_FUSE": "1"})))
    out.append(("grad one, float64 X", pass2_route(NXB_ROWS, 512, [(0, 256, GRAD_D)], cu, env={}, x64=True)))
    for name, rows, d in DET_CASES:
        F, kids = LAYOUTS[name]
        out.append(("grad %s x %d det" % (name, rows), pass2_route(rows, F, [(c0, n, d) for c0, n in kids], cu, det=True, env={})))
    for e in ENGINES:
        out.append(("grad one, %s" % e, pass2_route(NXB_ROWS, 512, [(0, 256, GRAD_D)], cu, engine=e, env={})))
        out.append(("grad one, %s again" % e, pass2_route(300, 512, [(0, 256, GRAD_D)], cu, engine=e, env={}, cb_ready=True)))
        out.append(("predict 700, %s" % e, predict_route(257, 700, 0, cu, engine=e, env={})))
    for F in F64_F:
        out += [("f64 %d" % F, f64_route([F64_CHILD[F]])), ("f64 %d predict" % F, f64_route([], pred=True))]
    for F in PRED_F:
        for rows in PRED_ROWS:
            for mode in PRED_MODES:
                out.append(("predict %d x %d %s" % (F, rows, mode), predict_route(rows, F, cu=cu, **_pred_mode(mode))))
    for rows, d, n in QT_FUSED:
        for ce in QT_CHUNKS:
            env = {"RR_PASS2_CHUNK_ROWS": ce} if ce else {}
            out.append(("basis %s chunk %s" % ((rows, d, n), ce), basis_route(rows, d, n, cu, env=env)))
            out.append(("basis %s chunk %s stored" % ((rows, d, n), ce), basis_route(rows, d, n, cu, env=dict(env, RR_PASS2_NO_FUSE="1"))))
    for rows, d, n, kw in QT_STORED:
        out.append(("basis %s %s" % ((rows, d, n), sorted(kw)), basis_route(rows, d, n, cu, env={}, **kw)))
    out.append(("basis %s" % (QT_BIG,), basis_route(*QT_BIG, cu=cu, env={})))
    for rows, d, n in QT_PREDICT:
        for form in (0, 1):
            out.append(("basis predict %s form %d" % ((rows, d, n), form), basis_route(rows, d, n, cu, pred=True, form=form, env={})))
    return out


def _pred_mode(mode):
    """predict_route's keywords (and the switches in force) of a PRED_MODES entry."""
    env = {}
    if mode == "form1 stored":
        env["RR_PREDICT_NO_FUSE"] = "1"
    if mode.endswith("no diag skip"):
        env["RR_PREDICT_NO_DIAG_SKIP"] = "1"
    return {"form": int(mode[4]), "det": mode == "form1 det", "c_dev": mode == "form0 device", "env": env}


# ---- exact data ---------------------------------------------------------------------------------------------------------
def _tern(rs, shape, p):
    return rs.choice(np.array([-1.0, 0.0, 1.0], dtype=np.float32), size=shape, p=[p / 2, 1 - p, p / 2])


def _posterior(rs, F):
    """m in {-2 .. 2} (nonzero with probability min(0.5, 6 / F)) and the symmetric integer C of the module docstring."""
    m = (rs.randint(1, 3, size=F) * rs.choice([-1, 1], size=F) * (rs.rand(F) < min(0.5, 6.0 / F))).astype(np.float64)
    up = np.triu(_tern(rs, (F, F), min(1.0, 3.0 / F)).astype(np.float64), 1)
    return m, up + up.T + np.diag(rs.randint(1, 3, size=F).astype(np.float64))


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _reference(Phi, m, C, y, kids, s=1.0):
    """(sqErr, [T per child (col0, n, X)]) of the second pass, with the conditions of the module docstring asserted in
    quanta: Phi / s, U / s and err / s are integers, T / s^2 too."""
    Pi = Phi.astype(np.float32) / np.float32(s)
    assert np.array_equal(Pi, np.rint(Pi))
    l1 = float(np.abs(Pi).sum(axis=1, dtype=np.float64).max())
    assert l1 * max(np.abs(C).max(), np.abs(m).max()) < EXACT, "U or dot may leave the exact range"
    Ui = Pi @ C.astype(np.float32)                                    # integers below 2^24 in any order: exact in float32 too
    erri = y.astype(np.float64) / s - (Pi @ m.astype(np.float32)).astype(np.float64)
    assert np.abs(erri).max() < EXACT and np.array_equal(erri, np.rint(erri))
    sq = float((erri * erri).sum()) * s * s
    e32 = erri.astype(np.float32)[:, None]
    Ts = []
    for col0, n, X in kids:
        Pc, Ps, Uc, Us = Pi[:, col0:col0 + n], Pi[:, col0 + n:col0 + 2 * n], Ui[:, col0:col0 + n], Ui[:, col0 + n:col0 + 2 * n]
        mc, ms = m[col0:col0 + n].astype(np.float32), m[col0 + n:col0 + 2 * n].astype(np.float32)
        W = np.abs(e32) * (np.abs(Pc) * np.abs(ms) + np.abs(Ps) * np.abs(mc)) + np.abs(Pc * Us) + np.abs(Ps * Uc)
        X32 = X.astype(np.float32)
        bound = float((np.abs(X32).T @ W).max())
        assert W.max() < EXACT and bound < EXACT, ("T may leave the exact range", bound)
        A = e32 * (Pc * ms - Ps * mc) - (Pc * Us - Ps * Uc)
        T = (X32.T @ A).astype(np.float64) * s * s
        nz = float((T != 0).mean())
        rows = Phi.shape[0]
        assert nz >= (0.95 if rows >= 1000 else 0.9 if rows >= 256 else 0.01), ("T is too sparse for == to mean much", nz)
        Ts.append(T)
    return sq, Ts


def _predict_reference(Phi, m, C=None, B=None, s=1.0):
    """(Ey, Vf): Vf = phi^T C phi (the device forms it through the triangular Ctri = diag + 2 triu) or |phi^T B|^2."""
    Pi = Phi.astype(np.float32) / np.float32(s)
    assert np.array_equal(Pi, np.rint(Pi))
    l1 = float(np.abs(Pi).sum(axis=1, dtype=np.float64).max())
    Ey = (Pi @ m.astype(np.float32)).astype(np.float64) * s
    if B is None:
        tri = np.triu(C, 1) * 2 + np.diag(np.diag(C))
        assert l1 * max(np.abs(tri).max(), np.abs(m).max()) < EXACT
        Ut = Pi @ tri.astype(np.float32)
        assert float((np.abs(Ut) * np.abs(Pi)).sum(axis=1, dtype=np.float64).max()) < EXACT
        Vf = ((Pi @ C.astype(np.float32)) * Pi).sum(axis=1, dtype=np.float64) * s * s
        assert np.array_equal(Vf, (Ut * Pi).sum(axis=1, dtype=np.float64) * s * s)
    else:
        assert l1 * max(np.abs(B).max(), np.abs(m).max()) < EXACT
        U = Pi @ B.astype(np.float32)
        Vf = (U * U).sum(axis=1, dtype=np.float64)
        assert Vf.max() < EXACT
        Vf = Vf * s * s
    assert (Vf != 0).all(), "a zero Vf"
    return Ey, Vf


class _GradCase(object):
    pass


def _make_grad_case(layout, rows, d, seed=0):
    F, kids = LAYOUTS[layout]
    rs = np.random.RandomState(zlib_seed(layout, rows, d, seed))
    g = _GradCase()
    g.layout, g.rows, g.F = layout, rows, F
    g.Phi = _tern(rs, (rows, F), 0.15)
    g.m, g.C = _posterior(rs, F)
    g.y = rs.randint(-3, 4, size=rows).astype(np.float64)
    g.kids = [(c0, n, rs.randint(-2, 3, size=(rows, d)).astype(np.float32)) for c0, n in kids]
    g.children = [(c0, n, d) for c0, n in kids]
    g.sq, g.T = _reference(g.Phi, g.m, g.C, g.y, g.kids)
    _frozen(g.Phi, g.m, g.C, g.y, *(g.T + [X for _, _, X in g.kids]))
    return g


def zlib_seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


_grad_case = functools.lru_cache(maxsize=6)(_make_grad_case)
_big_grad_case = functools.lru_cache(maxsize=2)(_make_grad_case)


@functools.lru_cache(maxsize=4)
def _pred_case(rows, F):
    rs = np.random.RandomState(zlib_seed("predict", rows, F))
    Phi = _tern(rs, (rows, F), 0.15)
    m, C = _posterior(rs, F)
    B = np.triu(_posterior(rs, F)[1])
    return _frozen(Phi, m, C, B, _predict_reference(Phi, m, C=C), _predict_reference(Phi, m, B=B))


# ---- running the device --------------------------------------------------------------------------------------------------
def _assert_bitwise(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d of %d differ, max |diff| %g, first at %s" % (
        what, int(bad.sum()), bad.size, np.abs(got - want).max(), tuple(int(i) for i in np.argwhere(bad)[0]))


def _device():
    from revrand_amd import _hip
    return _hip.get_device()


class _Env(object):
    """Per-call switches, deterministic mode and the engine for the duration of a block."""

    def __init__(self, env=None, det=False, engine=None):
        self.env, self.det, self.engine = dict(env or {}), det, engine

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in PER_CALL}
        for k in PER_CALL:
            os.environ.pop(k, None)
        os.environ.update(self.env)
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


def _prefill(d, n):
    i, j = np.indices((d, n))
    K = ((3 * i + 5 * j) % 13 - 6).astype(np.float64)
    K[K == 0] = 7.0          # integers, none zero: T is accumulated into, and `==` is never vacuous
    return K


def run_pass2(g, fm=None, env=None, det=False, engine=None, x64=False, y_dtype=np.float32, begin_pass=True, f64=False,
              count=None):
    """begin / put_host / pass2_begin / plan / rows_planned / pass2_rff / pass2_end of the case g on the feature matrix fm
    (default: a fresh one): (sqErr, [T per child]) with dT prefilled and the prefill taken off again.  begin_pass=False:
    another batch of rows under the posterior of the last pass2_begin (sqErr keeps accumulating).  f64: FeatureMatrix64
    (pass2_rows; no plans).  count: the library, to reset the launch counters before the first counted call."""
    from revrand_amd import _hip
    dev = _device()
    if fm is None:
        fm = (_hip.FeatureMatrix64 if f64 else _hip.FeatureMatrix)(g.rows, g.F)
    bufs, kids = [], []
    try:
        for col0, n, X in g.kids:
            h = _hip.RffHandle(np.zeros((X.shape[1], n)))
            dX = dev.upload_matrix(X.astype(np.float64 if x64 else np.float32), ld_dev=h.padded_dim)
            K = _prefill(X.shape[1], n)
            dT = dev.upload_vector(K)
            bufs += [dX, dT]
            kids.append((h, dX, col0, dT, K))
        dy = dev.upload_vector(g.y, dtype=y_dtype)
        bufs.append(dy)
        with _Env(env, det, engine):
            fm.begin(g.rows)
            fm.put_host(g.Phi if not f64 else g.Phi.astype(np.float64), 0)
            dev.sync()
            if count is not None:
                count.rr_debug_kernel_launches(None)
            if begin_pass:
                fm.pass2_begin(g.m, g.C)
            if f64:
                fm.pass2_rows(dy)
            else:
                for h, dX, col0, dT, K in kids:
                    fm.pass2_plan_rff(h, dX, col0, dT)
                fm.pass2_rows_planned(dy)
            for h, dX, col0, dT, K in kids:
                fm.pass2_rff(h, dX, col0, dT)
            sq = fm.pass2_end()
            Ts = [dev.download(dT, K.shape, np.float64) - K for h, dX, col0, dT, K in kids]
        return sq, Ts
    finally:
        for b in bufs:
            b.free()


def _check_pass2(g, what, **kw):
    sq, Ts = run_pass2(g, **kw)
    assert sq == g.sq, (what, "sqErr", sq, g.sq)
    for (col0, n, d), T, Tr in zip(g.children, Ts, g.T):
        _assert_bitwise(T, Tr, "%s: T of the child at column %d" % (what, col0))
    return sq, Ts


def run_predict(Phi, m, C=None, B=None, c_dev=False, fm=None, env=None, det=False, engine=None, f64=False, count=None):
    """(Ey, Vf) through pass2_begin(predict=True) (host C; c_dev: a device float64 C) or rr_featmat_predict_begin_b with
    the device float32 (Fp, Fp) factor B, form 1."""
    from revrand_amd import _hip
    dev = _device()
    rows, F = Phi.shape
    if fm is None:
        fm = (_hip.FeatureMatrix64 if f64 else _hip.FeatureMatrix)(rows, F)
    bufs = []
    try:
        with _Env(env, det, engine):
            fm.begin(rows)
            fm.put_host(Phi if not f64 else Phi.astype(np.float64), 0)
            dev.sync()
            if count is not None:
                count.rr_debug_kernel_launches(None)
            if B is not None:
                Fp = _up(F, 256)
                Bp = np.zeros((Fp, Fp), dtype=np.float32)
                Bp[:F, :F] = B
                dB = dev.upload_vector(Bp.ravel())
                bufs.append(dB)
                mm = np.ascontiguousarray(m, dtype=np.float64)
                _hip._check(fm.lib, fm.lib.rr_featmat_predict_begin_b(fm.h, mm.ctypes.data_as(_hip.ctypes.c_void_p), dB.ptr, 1))
            elif c_dev:
                dC = dev.upload_vector(np.ascontiguousarray(C, dtype=np.float64).ravel())
                bufs.append(dC)
                fm.pass2_begin(m, dC, predict=True)
            else:
                fm.pass2_begin(m, C, predict=True)
            return fm.predict_rows(rows)
    finally:
        for b in bufs:
            b.free()


def _check_predict(rows, F, mode, what=None, **kw):
    Phi, m, C, B, ref0, ref1 = _pred_case(rows, F)
    r = _pred_mode(mode)
    if r["form"] == 0:
        Ey, Vf = run_predict(Phi, m, C=C, c_dev=r["c_dev"], env=r["env"], det=r["det"], **kw)
        ref = ref0
    else:
        Ey, Vf = run_predict(Phi, m, B=B, env=r["env"], det=r["det"], **kw)
        ref = ref1
    what = what or "predict %d x %d, %s" % (rows, F, mode)
    _assert_bitwise(Ey, ref[0], what + ": Ey")
    _assert_bitwise(Vf, ref[1], what + ": Vf")
    return Ey, Vf


# ---- tests: the route table ----------------------------------------------------------------------------------------------
def test_cases_cover_every_route():
    """The cases of this module, routed by the tables at this device's CU count, reach every row of the route table of
    docs/KERNELS.md 3.5."""
    cu = _device().compute_units
    hit = {}
    for label, r in route_cases(cu):
        keys = []
        k = r["kernels"]
        for g in r.get("gradt", []):
            keys += ["gradt NXB = %d" % g["nxb"], "gradt ntb = %d" % g["ntb"]]
            if g["walk"] >= 2 and g["partial"]:
                keys.append("gradt: a workgroup walks >= 2 row tiles, the last one partial")
            if g["walk"] >= 2:
                keys.append("gradt NXB = %d over >= 2 row tiles" % g["nxb"])
            if g["nta"] == 1 and g["partial"]:
                keys.append("gradt: one partial row tile")
        if "f64" in r:
            keys.append("float64 %s" % r["f64"])
        elif "ld" in r:     # feature-matrix gradient pass
            keys.append("featmat gradient %s" % ("fused" if r["fused"] else "stored"))
            if r["fused"] and r["live_last_kblock"] < 32:
                keys.append("gradt: %d live rows in the last k-block" % r["live_last_kblock"])
            if r["fused"] and len(r["gradt"]) == 2:
                keys.append("gradt: two planned children, columns nobody consumes")
            for dm in r.get("dm", []):
                keys.append("grad_t DM = %d" % dm if dm else "grad_t Xdim > 128: %d launches" % k["rr_grad_t_kernel"])
            if k["rr_syrk_b16w4_kernel"]:
                keys.append("gradient on a split engine, C %s" % ("reused" if k["rr_split_bf16_kernel"] == 1 else "converted"))
        elif "chunks" in r:   # single basis
            what = "basis predict" if (k["rr_rowdot_kernel"] or r["fused_vf"]) and not k["rr_err_kernel"] else "basis gradient"
            keys += ["%s, features by %s" % (what, f) for f in r["features"]]
            if what == "basis gradient":
                keys.append("basis gradient %s" % ("fused" if r["fused"] else "stored"))
                if len(r["chunks"]) > 1 and r["chunks"][-1] % 256:
                    keys.append("basis gradient %s: several chunks, a partial last one" % ("fused" if r["fused"] else "stored"))
                if not r["fused"]:
                    keys.append("basis grad_t DM = %d" % r["dm"] if r["dm"] else "basis grad_t Xdim > 128: %d launches" % k["rr_grad_t_kernel"])
            else:
                keys.append("basis predict, %s" % ("rowsq epilogue, no row-major P" if not r["need_p"] else "rowdot"))
        else:
            keys.append("predict %s, %s column tiles" % ("pair kernel" if r["pair"] else "gemm_tn upper_b" if k["rr_gemm_tn_f32_kernel"] else "split engine", r["pairs"]))
            keys.append("predict form %d, Vf by %s" % (r["form"], "rowsq epilogue" if r["fused_vf"] else "rowdot"))
            if r["pair"] and not r["diag_skip"]:
                keys.append("predict pair kernel without the diagonal skip")
            if k["rr_c64_to_c32_kernel"]:
                keys.append("predict C from the device (c64_to_c32, tri)")
        for key in keys:
            hit.setdefault(key, label)
    for key in sorted(hit):
        print("%-72s %s" % (key, hit[key]))
    want = {"gradt NXB = 1", "gradt NXB = 2", "gradt NXB = 4", "gradt ntb = 2", "gradt ntb = 8",
            "gradt: a workgroup walks >= 2 row tiles, the last one partial", "gradt NXB = 1 over >= 2 row tiles",
            "gradt NXB = 2 over >= 2 row tiles", "gradt: one partial row tile", "featmat gradient fused", "featmat gradient stored",
            "gradt: 3 live rows in the last k-block", "gradt: two planned children, columns nobody consumes",
            "grad_t DM = 8", "grad_t DM = 16", "grad_t DM = 32", "grad_t DM = 64", "grad_t DM = 128", "grad_t Xdim > 128: 2 launches",
            "gradient on a split engine, C converted", "gradient on a split engine, C reused",
            "basis gradient fused", "basis gradient stored", "basis gradient, features by t4", "basis gradient, features by t",
            "basis gradient, features by transpose", "basis gradient fused: several chunks, a partial last one",
            "basis gradient stored: several chunks, a partial last one", "basis grad_t DM = 8", "basis grad_t DM = 16",
            "basis grad_t DM = 32", "basis grad_t DM = 64", "basis grad_t DM = 128", "basis grad_t Xdim > 128: 2 launches",
            "basis predict, features by t4", "basis predict, features by transpose", "basis predict, rowsq epilogue, no row-major P",
            "basis predict, rowdot",
            "predict pair kernel, one tile column tiles", "predict pair kernel, even column tiles", "predict pair kernel, odd column tiles",
            "predict split engine, odd column tiles", "predict form 0, Vf by rowdot", "predict form 1, Vf by rowsq epilogue",
            "predict form 1, Vf by rowdot", "predict pair kernel without the diagonal skip", "predict C from the device (c64_to_c32, tri)", "float64 gradient", "float64 predict"}
    assert want <= set(hit), sorted(want - set(hit))
    # the row-tile walks the issue names, at the MI355X's 256 CUs (on another CU count the assertion above still holds them)
    if cu == 256:
        assert gradt_geometry(9000, 1024, 40, cu)["G"] == 32 and gradt_geometry(9000, 1024, 40, cu)["nta"] == 36
        assert gradt_geometry(40000, 256, 8, cu)["G"] == 128 and gradt_geometry(40000, 256, 8, cu)["nta"] == 157
        assert basis_route(*QT_BIG, cu=cu, env={})["features"] == {"t"}
    # the triangular product without the pair kernel belongs to a switch read at process start: the child's cases reach it
    off = {"RR_PREDICT_NO_PAIR": "1"}
    assert all(predict_route(rows, F, 0, cu, env=off)["kernels"]["rr_gemm_tn_f32_kernel"] == 1 for rows, F, mode in STATIC_PREDICT)
    assert {predict_route(rows, F, 0, cu, env=off)["ntb"] for rows, F, mode in STATIC_PREDICT} >= {1, 3, 5}
    assert any(basis_route(r, d, n, cu, env={"RR_FEATURES_T_NO_SPLIT": "1"})["features"] == {"t"} for r, d, n in QT_FUSED)
    assert all(basis_route(r, d, n, cu, pred=True, form=1, env={"RR_PREDICT_NO_FUSE": "1"})["need_p"] for r, d, n in QT_PREDICT)


# ---- tests: the gradient pass of a feature matrix ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", GRAD_ROWS)
@pytest.mark.parametrize("layout", SWEEP_LAYOUTS)
def test_gradient_pass_is_exact(layout, rows):
    """sqErr and every child's T on each layout and row count (one row, part tiles, whole tiles, one row past a tile, 20
    tiles with a partial last one): the route the driver takes, the stored route at the same shape (RR_PASS2_NO_FUSE=1),
    one reference, and the two routes against each other."""
    g = _grad_case(layout, rows, GRAD_D)
    assert pass2_route(rows, g.F, g.children, _device().compute_units, env={})["fused"] == (layout in FUSED_LAYOUTS)
    _, Ta = _check_pass2(g, "grad %s x %d" % (layout, rows))
    _, Tb = _check_pass2(g, "grad %s x %d stored" % (layout, rows), env={"RR_PASS2_NO_FUSE": "1"})
    for a, b in zip(Ta, Tb):
        _assert_bitwise(a, b, "fused against stored")
    _check_pass2(g, "grad %s x %d, float64 y" % (layout, rows), y_dtype=np.float64)


@pytest.mark.parametrize("layout,rows,d", BIG_GRAD)
def test_gradient_pass_with_more_row_tiles_than_workgroups_is_exact(layout, rows, d):
    """nta > G: every workgroup of the fused kernel walks two row tiles (g, g + G), some a partial last one, T kept in
    registers across them (NXB = 1, d = 8) or flushed per tile (NXB = 2, d = 40); against the stored route too."""
    g = _big_grad_case(layout, rows, d)
    _, Ta = _check_pass2(g, "grad %s x %d" % (layout, rows))
    _, Tb = _check_pass2(g, "grad %s x %d stored" % (layout, rows), env={"RR_PASS2_NO_FUSE": "1"})
    _assert_bitwise(Ta[0], Tb[0], "fused against stored")


@pytest.mark.parametrize("d", sorted(set(NXB_D + DM_D)))
def test_gradient_pass_over_the_input_dimensions_is_exact(d):
    """NXB = 1, 2, 4 of the fused kernel with whole and partial last 32-column blocks of X, and DM = 8 .. 128 of
    rr_grad_t_kernel; Xdim = 130 (stored only): 128 + 2 dimensions in two launches."""
    g = _grad_case("one", NXB_ROWS, d)
    if d <= 128:
        _check_pass2(g, "grad d = %d" % d)
    _check_pass2(g, "grad d = %d stored" % d, env={"RR_PASS2_NO_FUSE": "1"})


def test_gradient_pass_with_float64_inputs_is_exact():
    """A float64 X takes the stored route (rr_grad_t_kernel<DM, double>) whatever the layout."""
    _check_pass2(_grad_case("one", NXB_ROWS, GRAD_D), "grad float64 X", x64=True, y_dtype=np.float64)


@pytest.mark.parametrize("layout,rows,d", DET_CASES)
def test_gradient_pass_in_deterministic_mode_is_exact_and_repeats(layout, rows, d):
    """Deterministic mode: the stored route with sqErr and T through ordered slabs; the exact result, twice."""
    g = _grad_case(layout, rows, d)
    a = _check_pass2(g, "grad %s x %d det" % (layout, rows), det=True)
    b = _check_pass2(g, "grad %s x %d det again" % (layout, rows), det=True)
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        _assert_bitwise(x, y, "repeat")


@pytest.mark.parametrize("env", [{}, {"RR_PASS2_NO_FUSE": "1"}], ids=["fused", "stored"])
@pytest.mark.parametrize("layout", ["one", "two+linear"])
def test_one_feature_matrix_through_shrinking_row_counts(layout, env):
    """1000 -> 37 -> 300 rows on one FeatureMatrix: no result sees the stale rows of P, P^T, U or err of the taller batch."""
    from revrand_amd import _hip
    fm = _hip.FeatureMatrix(max(REUSE_ROWS), LAYOUTS[layout][0])
    for step, rows in enumerate(REUSE_ROWS):
        _check_pass2(_grad_case(layout, rows, GRAD_D), "step %d (%d rows)" % (step, rows), fm=fm, env=env)


def test_gradient_pass_with_a_child_that_wrote_its_transpose():
    """A quarter-turn random Fourier child put by put_rff next to P^T (`fm->pt_covered`: after one transposing pass at this
    row count the children write P^T themselves and the pass skips its transpose): the same exact results."""
    from revrand_amd import _hip
    rows, d, n = 1000, 5, 256
    q = _qt_case(rows, d, n)
    dev = _device()
    h = _hip.RffHandle(q.W)
    fm = _hip.FeatureMatrix(rows, 2 * n)
    dX = h.upload(q.X)
    dy = dev.upload_vector(q.y, dtype=np.float32)
    try:
        for step in range(2):     # the first pass lays out P^T's padding, the second one finds P^T written
            dT = dev.zeros(d * n * 8)
            with _Env():
                fm.begin(rows)
                fm.put_rff(h, dX, 1.0, 0)
                _assert_bitwise(fm.download(), q.Phi, "step %d: the features" % step)
                fm.pass2_begin(q.m, q.C)
                fm.pass2_plan_rff(h, dX, 0, dT)
                fm.pass2_rows_planned(dy)
                fm.pass2_rff(h, dX, 0, dT)
                sq = fm.pass2_end()
            T = dev.download(dT, (d, n), np.float64)
            dT.free()
            assert sq == q.sq, (step, sq, q.sq)
            _assert_bitwise(T, q.T, "step %d: T" % step)
    finally:
        dX.free()
        dy.free()


# ---- tests: prediction on a feature matrix ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", PRED_ROWS)
@pytest.mark.parametrize("F", PRED_F)
def test_prediction_is_exact(F, rows):
    """Ey = Phi m and Vf = phi^T C phi (form 0: host C and a device float64 C) or |phi^T B|^2 (form 1: summed in the product's
    epilogue, stored and reduced by rr_rowdot_kernel, deterministic mode) at one to five column tiles -- pairs (q, ntb - 1 - q)
    with an odd and an even count --, with and without the skipped zero quarters of the diagonal blocks."""
    for mode in PRED_MODES:
        _check_predict(rows, F, mode)


def test_one_feature_matrix_predicts_shrinking_row_counts():
    from revrand_amd import _hip
    fm = _hip.FeatureMatrix(1000, 700)
    for rows in (1000, 37, 257):
        for mode in ("form0 host", "form1 fused", "form1 stored"):
            _check_predict(rows, 700, mode, fm=fm)


# ---- tests: the split engines -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_split_engines_are_exact(engine):
    """U = Phi C through rr_launch_gemm_tn_bf16: ternary features and small integers have a zero low part, so the exact
    result is the integer one; a second batch of rows under the same posterior reuses the converted C (`cb_ready`), and
    sqErr and T keep accumulating."""
    from revrand_amd import _hip
    g, g2 = _grad_case("one", NXB_ROWS, GRAD_D), _grad_case("one", 300, GRAD_D)
    fm = _hip.FeatureMatrix(NXB_ROWS, g.F)
    _check_pass2(g, "grad %s" % engine, fm=fm, engine=engine)
    g3 = _GradCase()
    g3.__dict__.update(g2.__dict__)
    g3.m, g3.C = g.m, g.C                       # the second batch under the first posterior
    g3.sq, g3.T = _reference(g3.Phi, g3.m, g3.C, g3.y, g3.kids)
    sq, Ts = run_pass2(g3, fm=fm, engine=engine, begin_pass=False)
    assert sq == g.sq + g3.sq
    _assert_bitwise(Ts[0], g3.T[0], "%s, second batch: T" % engine)
    for mode in ("form0 host", "form1 fused"):
        _check_predict(257, 700, mode, what="predict %s %s" % (engine, mode), engine=engine)


# ---- tests: float64 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _case64(rows, F):
    rs = np.random.RandomState(zlib_seed("f64", rows, F))
    col0, n, d = F64_CHILD[F]
    g = _GradCase()
    g.rows, g.F, g.children = rows, F, [(col0, n, d)]
    P = rs.randint(-1000, 1001, size=(rows, F)).astype(np.float64)
    g.Phi = P
    g.m = rs.randint(-10, 11, size=F).astype(np.float64)
    up = np.triu(rs.randint(-10, 11, size=(F, F)).astype(np.float64), 1)
    g.C = up + up.T + np.diag(rs.randint(1, 11, size=F).astype(np.float64))
    g.y = rs.randint(-1000, 1001, size=rows).astype(np.float64)
    X = rs.randint(-100, 101, size=(rows, d)).astype(np.float64)
    g.kids = [(col0, n, X)]
    dot, U = P @ g.m, P @ g.C
    err = g.y - dot
    Pc, Ps, Uc, Us = P[:, col0:col0 + n], P[:, col0 + n:col0 + 2 * n], U[:, col0:col0 + n], U[:, col0 + n:col0 + 2 * n]
    mc, ms = g.m[col0:col0 + n], g.m[col0 + n:col0 + 2 * n]
    W = np.abs(err)[:, None] * (np.abs(Pc) * np.abs(ms) + np.abs(Ps) * np.abs(mc)) + np.abs(Pc * Us) + np.abs(Ps * Uc)
    big = max((np.abs(P) @ np.abs(g.C)).max(), (np.abs(P) @ np.abs(g.m)).max(), (np.abs(X).T @ W).max(), (err * err).sum(),
              (np.abs(U) * np.abs(P)).sum(axis=1).max())
    assert EXACT < big < 2.0 ** 53, big           # exact in float64, out of reach of any float32 step
    g.sq = float(err @ err)
    g.T = [X.T @ (err[:, None] * (Pc * ms - Ps * mc) - (Pc * Us - Ps * Uc))]
    g.Ey, g.Vf = dot, (U * P).sum(axis=1)
    assert (g.Vf != 0).all() and (g.T[0] != 0).mean() > 0.95
    return g


@pytest.mark.parametrize("rows", F64_ROWS)
@pytest.mark.parametrize("F", F64_F)
def test_feature_matrix64_is_exact(F, rows):
    """FeatureMatrix64's pass2_rows / pass2_rff / predict_rows (fm64_products, rr_rows64_kernel<0 | 1>, rr_err64_kernel,
    rr_grad_t64_kernel, rr_gemm_tn_f64_kernel) on integers far above 2^24: float32 and float64 X and y, deterministic
    mode and not, a host and a device C."""
    g = _case64(rows, F)
    for x64 in (False, True):
        for det in (False, True):
            _check_pass2(g, "f64 %s x64=%s det=%s" % ((rows, F), x64, det), f64=True, x64=x64, det=det,
                         y_dtype=np.float64 if x64 else np.float32)
    for c_dev in (False, True):
        Ey, Vf = run_predict(g.Phi, g.m, C=g.C, c_dev=c_dev, f64=True)
        _assert_bitwise(Ey, g.Ey, "f64 %s: Ey" % ((rows, F),))
        _assert_bitwise(Vf, g.Vf, "f64 %s: Vf" % ((rows, F),))


# ---- part 2: one random Fourier basis at quarter turns -----------------------------------------------------------------------
class _QtCase(object):
    pass


def _make_qt_case(rows, d, n, density=0.1):
    """X ternary, W = (pi / 2) Q: the features are exactly cos / sin of k quarter turns, k = (X Q) mod 4, over sqrt(n)."""
    rs = np.random.RandomState(zlib_seed("qt", rows, d, n))
    q = _QtCase()
    q.rows, q.d, q.n = rows, d, n
    s = 1.0 / np.sqrt(n)
    assert s == 2.0 ** round(np.log2(s)), "1 / sqrt(n) must be a power of two"
    q.s = s
    q.X = _tern(rs, (rows, d), density)
    Q = rs.randint(-3, 4, size=(d, n)).astype(np.float64)
    q.W = (np.pi / 2) * Q
    assert np.array_equal((q.W / (2 * np.pi)).astype(np.float32), (Q / 4).astype(np.float32))
    Z = q.X.astype(np.float64) @ Q
    assert np.abs(Z).max() / 4 < 256         # revolutions, against the instructions' +-256
    k = np.mod(Z, 4).astype(np.int64)
    cos, sin = np.array([1.0, 0.0, -1.0, 0.0])[k], np.array([0.0, 1.0, 0.0, -1.0])[k]
    q.Phi = (np.hstack([cos, sin]) * s).astype(np.float32)
    q.classes = np.bincount(k.ravel(), minlength=4)
    for blk in range(0, 2 * n, 32):          # both halves keep nonzero columns in every 32-column block
        assert np.abs(q.Phi[:, blk:blk + 32]).sum() > 0
    q.m, q.C = _posterior(rs, 2 * n)
    q.B = np.triu(_posterior(rs, 2 * n)[1])
    q.y = rs.randint(-2, 3, size=rows).astype(np.float64)
    q.sq, (q.T,) = _reference(q.Phi, q.m, q.C, q.y, [(0, n, q.X)], s=s)
    return q


_qt_cached = functools.lru_cache(maxsize=4)(_make_qt_case)


def _qt_case(rows, d, n):
    """10 % dense X; 5 % at Xdim > 128, which keeps the phases within a few revolutions."""
    return _qt_cached(rows, d, n, 0.05 if d > 128 else 0.1)


_qt_big_case = functools.lru_cache(maxsize=1)(_make_qt_case)


def _qt_probe(q):
    """'' or what is wrong with the device features of the quarter-turn case q (transform, and put_rff + download)."""
    from revrand_amd import _hip
    h = _hip.RffHandle(q.W)
    P = h.transform(q.X, 1.0, out_dtype=np.float32)
    bad = []
    vals = set(np.unique(P).tolist())
    if not vals <= {0.0, q.s, -q.s}:
        bad.append("transform: values %s" % sorted(vals - {0.0, q.s, -q.s})[:8])
    if not np.array_equal(P, q.Phi):
        bad.append("transform: %d entries differ from the exact features" % int((P != q.Phi).sum()))
    fm = _hip.FeatureMatrix(q.rows, 2 * q.n)
    dX = h.upload(q.X)
    try:
        fm.begin(q.rows)
        fm.put_rff(h, dX, 1.0, 0)
        D = fm.download()[:, :2 * q.n]
    finally:
        dX.free()
    if not np.array_equal(D, q.Phi):
        bad.append("put_rff: %d entries differ, values %s" % (int((D != q.Phi).sum()), sorted(set(np.unique(D).tolist()) - {0.0, q.s, -q.s})[:8]))
    return "; ".join(bad)


QT_PROBE = sorted({(r, d, n) for r, d, n in QT_FUSED + QT_PREDICT} | {(r, d, n) for r, d, n, kw in QT_STORED if not kw})


@pytest.mark.parametrize("rows,d,n", QT_PROBE)
def test_quarter_turn_features_are_exact(rows, d, n):
    """v_cos_f32 / v_sin_f32 at k / 4 revolutions (all four classes occur, phases up to a few revolutions): every feature
    of every quarter-turn case is exactly 0 or +-1 / sqrt(n), through the row-major feature kernels of RffHandle.transform
    and of FeatureMatrix.put_rff.  Everything below in part 2 rests on this."""
    q = _qt_case(rows, d, n)
    assert (q.classes > 0).all(), q.classes
    assert _qt_probe(q) == ""


def run_basis_pass2(q, h=None, env=None, det=False, x64=False, compute="f32", c_dev=False):
    from revrand_amd import _hip
    dev = _device()
    h = h or _hip.RffHandle(q.W, compute=compute)
    xt = np.float64 if x64 or h.x_dtype == np.float64 else np.float32
    dX = h.upload(q.X.astype(xt))
    dy = dev.upload_vector(q.y, dtype=xt)
    dC = dev.upload_vector(q.C.ravel()) if c_dev else None
    try:
        with _Env(env, det):
            return h.elbo_pass2(dX, dy, 1.0, q.m, dC if c_dev else q.C)
    finally:
        dX.free()
        dy.free()
        if dC is not None:
            dC.free()


def _check_basis(q, what, **kw):
    sq, T = run_basis_pass2(q, **kw)
    assert sq == q.sq, (what, "sqErr", sq, q.sq)
    _assert_bitwise(T, q.T, what + ": T")
    return T


@pytest.mark.parametrize("rows,d,n", QT_FUSED)
def test_basis_gradient_pass_is_exact(rows, d, n):
    """RffHandle.elbo_pass2 (pass2_run): the feature-major kernels, the fused kernel at NXB = 1, 2, 4 and the stored route,
    in one chunk, in 768-row and in 256-row chunks with a partial last one -- on ONE handle, so that the smaller chunks
    run in the scratch (lda = chunk) of the larger call --, C from the host and from the device."""
    from revrand_amd import _hip
    q = _qt_case(rows, d, n)
    h = _hip.RffHandle(q.W)
    for ce in QT_CHUNKS:
        env = {"RR_PASS2_CHUNK_ROWS": ce} if ce else {}
        a = _check_basis(q, "basis %s chunk %s" % ((rows, d, n), ce), h=h, env=env)
        b = _check_basis(q, "basis %s chunk %s stored" % ((rows, d, n), ce), h=h, env=dict(env, RR_PASS2_NO_FUSE="1"))
        _assert_bitwise(a, b, "fused against stored")
    _check_basis(q, "basis %s, device C" % ((rows, d, n),), h=h, c_dev=True)


@pytest.mark.parametrize("rows,d,n,kw", QT_STORED, ids=lambda v: "+".join(sorted(v)) or "f32" if isinstance(v, dict) else str(v))
def test_basis_stored_routes_are_exact(rows, d, n, kw):
    """What only the stored route serves: n = 16 and 64 (one 256-column tile, mostly padding), float64 X, float64 phases
    (f32p64: row-major features, transposed), Xdim = 130 (5 % dense; the phase GEMM and two contraction launches),
    deterministic mode."""
    q = _qt_case(rows, d, n)
    assert not basis_route(rows, d, n, _device().compute_units, env={}, **kw)["fused"]
    if kw or d > 128:
        assert _qt_probe_compute(q, kw.get("compute", "f32")) == ""
    _check_basis(q, "basis %s %s" % ((rows, d, n), kw), **kw)


def _qt_probe_compute(q, compute):
    from revrand_amd import _hip
    P = _hip.RffHandle(q.W, compute=compute).transform(q.X, 1.0, out_dtype=np.float32)
    return "" if np.array_equal(P, q.Phi) else "transform (%s): %d entries differ" % (compute, int((P != q.Phi).sum()))


def test_basis_gradient_pass_through_the_plain_feature_major_kernel_is_exact():
    """131 328 rows: 513 row tiles, from which launch_features_t takes rr_rff_features_t_kernel rather than its split form
    on 256 CUs; the fused kernel walks three row tiles per workgroup."""
    q = _qt_big_case(*QT_BIG)
    _check_basis(q, "basis %s" % (QT_BIG,))


def run_basis_predict(q, what, h=None, env=None, det=False):
    """(Ey, Vf) of q.X through RffHandle.predict with C (form 0), rr_rff_predict_devb with the device factor B (form 1),
    or the mean-only kernel (C = None)."""
    from revrand_amd import _hip
    dev = _device()
    h = h or _hip.RffHandle(q.W)
    with _Env(env, det):
        if what == "form0":
            return h.predict(q.X, 1.0, q.m, q.C)
        if what == "mean":
            return h.predict(q.X, 1.0, q.m, None)
        F, Fp = 2 * q.n, _up(2 * q.n, 256)
        Bp = np.zeros((Fp, Fp), dtype=np.float32)
        Bp[:F, :F] = q.B
        dB, dX = dev.upload_vector(Bp.ravel()), h.upload(q.X)
        try:
            Ey, Vf = np.empty(q.rows), np.empty(q.rows)
            ls, lsp, nls = _hip._lenscale_arg(1.0)
            vp = _hip.ctypes.c_void_p
            _hip._check(h.lib, h.lib.rr_rff_predict_devb(h.h, dX.ptr, _hip.rr_dtype(dX.dtype), q.rows, dX.ld, lsp, nls,
                                                         q.m.ctypes.data_as(vp), dB.ptr, 1, Ey.ctypes.data_as(vp), Vf.ctypes.data_as(vp)))
            return Ey, Vf
        finally:
            dB.free()
            dX.free()


def _check_basis_predict(q, h=None, det=False):
    ref0, ref1 = _predict_reference(q.Phi, q.m, C=q.C, s=q.s), _predict_reference(q.Phi, q.m, B=q.B, s=q.s)
    E0, V0 = run_basis_predict(q, "form0", h, det=det)
    E1, V1 = run_basis_predict(q, "form1", h, det=det)
    tag = "basis predict %s%s" % ((q.rows, q.d, q.n), " det" if det else "")
    _assert_bitwise(E0, ref0[0], tag + ": Ey, form 0")
    _assert_bitwise(V0, ref0[1], tag + ": Vf, form 0")
    _assert_bitwise(E1, ref1[0], tag + ": Ey, form 1")
    _assert_bitwise(V1, ref1[1], tag + ": Vf, form 1")
    if q.d <= 128:
        Em, none = run_basis_predict(q, "mean", h)
        assert none is None
        _assert_bitwise(Em, ref0[0], tag + ": Ey of the mean-only kernel")


@pytest.mark.parametrize("rows,d,n", QT_PREDICT)
def test_basis_prediction_is_exact(rows, d, n):
    """RffHandle.predict with C (form 0), rr_rff_predict_devb with a device factor (form 1: the squares summed in the
    product's epilogue, no row-major P -- `need_p` false) and the mean-only kernel: Ey of all three bit-identical, Vf
    exact; Xdim = 130 keeps its row-major P (the phase GEMM); deterministic mode takes the stored reduction."""
    q = _qt_case(rows, d, n)
    _check_basis_predict(q)
    if (rows, d, n) == QT_PREDICT[0]:
        _check_basis_predict(q, det=True)


# ---- the switches read once per process: one child each ----------------------------------------------------------------------
STATIC_PREDICT = [(257, 200, "form0 host"), (1000, 700, "form0 host"), (257, 700, "form1 fused"), (37, 1100, "form0 device"),
                  (1000, 1100, "form1 fused"), (257, 1280, "form1 stored")]
STATIC_GRAD = [("one", 257, 8), ("two+linear", 1000, 8), ("n150", 1000, 8)]
CHILD_TIMEOUT = 300


def statics_child():
    """A handful of the cases above under this process' environment: the list of mismatches (empty: all exact)."""
    bad = []

    def attempt(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except AssertionError as e:
            bad.append(str(e)[:400])

    for rows, F, mode in STATIC_PREDICT:
        attempt(_check_predict, rows, F, mode)
    for layout, rows, d in STATIC_GRAD:
        attempt(_check_pass2, _grad_case(layout, rows, d), "grad %s x %d" % (layout, rows))
    for rows, d, n in QT_FUSED[:3]:
        q = _qt_case(rows, d, n)
        attempt(_check_basis, q, "basis %s" % ((rows, d, n),))
        attempt(_check_basis, q, "basis %s stored" % ((rows, d, n),), env={"RR_PASS2_NO_FUSE": "1"})
    for rows, d, n in QT_PREDICT[:3]:
        attempt(_check_basis_predict, _qt_case(rows, d, n))
    return bad


CHILD_CODE = "import test_gpu_pass2_exact as S\n"


@pytest.mark.parametrize("variant", STATICS, ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()))
def test_switches_read_at_process_start_are_exact(monkeypatch, variant):
    """RR_PREDICT_NO_PAIR (the triangular product on rr_gemm_tn_f32_kernel with `upper_b`, its column tiles rotated by the
    row tile), RR_FEATURES_T_NO_SPLIT (the plain feature-major kernel at every row count) and pass2_run's RR_PREDICT_NO_FUSE
    (form 1 stored, with its row-major P) give the same exact results.  One child process after another, each under its own
    time limit; none is started after one that failed, timed out or reported a bounds violation (`guarded_child`)."""
    for k in STATIC_NAMES + list(PER_CALL):
        monkeypatch.delenv(k, raising=False)
    got = guarded_child(variant, CHILD_CODE + "print('P2RESULT', json.dumps(S.statics_child()))\n", variant, "P2RESULT",
                        timeout=CHILD_TIMEOUT, forbidden=("RR_BOUNDS",))
    assert got == []


# ---- which kernel ran (the bounds-checking build's launch counts; tests/test_debug_builds.py) -------------------------------
def census():
    """Launches of the kernels in KERNELS during one call per case under a library that counts them
    (rr_debug_kernel_launches), next to what the route tables predict, and whether the call's result was exact:
    [(label, compute units, {kernel: launches}, {kernel: predicted}, '' or the mismatch)]."""
    from revrand_amd import _hip
    dev = _device()
    lib, cu = dev.lib, dev.compute_units
    assert lib.rr_debug_kernel_launches(None) == 0
    out = []

    def counted():
        dev.sync()
        return {k: int(lib.rr_debug_kernel_launches(k.encode())) for k in KERNELS}

    def record(label, want, fn, *a, **kw):
        wrong = ""
        try:
            fn(*a, **kw)
        except AssertionError as e:
            wrong = str(e)[:300]
        out.append((label, cu, counted(), want, wrong))

    def grad(layout, rows, d, env=None, det=False, engine=None, x64=False):
        g = _grad_case(layout, rows, d)
        e = dict(env or {})
        want = pass2_route(rows, g.F, g.children, cu, engine=engine or "f32", det=det, env=e, x64=x64)["kernels"]
        record("grad %s x %d d=%d %s%s%s%s" % (layout, rows, d, sorted(e), " det" if det else "", " " + engine if engine else "",
                                              " x64" if x64 else ""), want, _check_pass2, g, "census", env=e, det=det,
               engine=engine, x64=x64, count=lib)

    for layout in SWEEP_LAYOUTS:
        for rows in (37, 1000):
            grad(layout, rows, GRAD_D)
            grad(layout, rows, GRAD_D, env={"RR_PASS2_NO_FUSE": "1"})
    for d in (33, 100):
        grad("one", NXB_ROWS, d)
    grad("one", NXB_ROWS, 130, env={"RR_PASS2_NO_FUSE": "1"})
    grad("one", NXB_ROWS, GRAD_D, x64=True)
    for layout, rows, d in DET_CASES:
        grad(layout, rows, d, det=True)
    for e in ENGINES:
        grad("one", NXB_ROWS, GRAD_D, engine=e)
    for F in PRED_F:
        for rows in (37, 1000):
            for mode in PRED_MODES:
                r = _pred_mode(mode)
                want = predict_route(rows, F, cu=cu, **r)["kernels"]
                record("predict %d x %d %s" % (F, rows, mode), want, _check_predict, rows, F, mode, count=lib)
    for F in F64_F:
        g = _case64(500, F)
        record("f64 500 x %d" % F, f64_route(g.children)["kernels"], _check_pass2, g, "census", f64=True, x64=True,
               y_dtype=np.float64, count=lib)
        lib.rr_debug_kernel_launches(None)
        record("f64 500 x %d predict" % F, f64_route([], pred=True)["kernels"], run_predict, g.Phi, g.m, C=g.C, f64=True)
    want = predict_route(257, 700, 0, cu, engine="bf16x3", env={})["kernels"]
    record("predict 700 x 257 bf16x3", want, _check_predict, 257, 700, "form0 host", engine="bf16x3", count=lib)
    for rows, d, n in QT_FUSED:
        q = _qt_case(rows, d, n)
        for env in ({}, {"RR_PASS2_NO_FUSE": "1"}, {"RR_PASS2_CHUNK_ROWS": "768"}):
            want = basis_route(rows, d, n, cu, env=dict(os.environ, **env))["kernels"]
            lib.rr_debug_kernel_launches(None)
            record("basis %s %s" % ((rows, d, n), sorted(env)), want, _check_basis, q, "census", env=env)
    for rows, d, n, kw in QT_STORED:
        q = _qt_case(rows, d, n)
        want = basis_route(rows, d, n, cu, env=dict(os.environ), **kw)["kernels"]
        lib.rr_debug_kernel_launches(None)
        record("basis %s %s" % ((rows, d, n), sorted(kw)), want, _check_basis, q, "census", **kw)
    for rows, d, n in QT_PREDICT:
        q = _qt_case(rows, d, n)
        for form in (0, 1):
            want = basis_route(rows, d, n, cu, pred=True, form=form, env=dict(os.environ))["kernels"]
            lib.rr_debug_kernel_launches(None)
            record("basis predict %s form %d" % ((rows, d, n), form), want, run_basis_predict, q, "form%d" % form)
    return out
