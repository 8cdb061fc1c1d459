"""CPU checks behind tests/test_gpu_fastfood_gm_wide.py: the recorded reference agrees with the oracle, the case list reaches
every instance of the wide chain kernel's mixture mode, the integer data stays exact with the mean shift added, the
``wide_chain`` keyword of FastFoodGM does what it says without a device, and the new entry point's signature is the old one's."""
import pickle

import numpy as np
import pytest

import revrand_oracle as orc
from conftest import load_golden, normwise

import fastfood_gm_wide_cases as gc
import fastfood_wide_cases as wc
from test_gpu_fastfood_exact import EXACT

GOLDEN_SHAPES = [(300, 600, 4), (1000, 1500, 3), (2049, 4097, 2), (4096, 4096, 2)]


@pytest.mark.parametrize("shape", GOLDEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_golden_file_against_the_oracle(shape):
    """tests/golden/fastfood_gm_wide.npz (the reference's outputs, tools/make_fastfood_gm_wide_golden.py) against the oracle on
    the stored inputs, at the stored columns: 1e-12 normwise."""
    d, nb, N = shape
    g = load_golden("fastfood_gm_wide")
    tag = "d%d" % d
    X = g["X_" + tag].astype(np.float64)
    assert X.shape == (N, d) and g["X_" + tag].dtype == np.float32
    cols, ard, mean = g["cols_" + tag], g["ls_ard_" + tag], g["mean_" + tag]
    assert np.array_equal(mean, 0.3 * np.random.RandomState(2000 + d).randn(d)) and np.array_equal(ard, np.linspace(0.7, 1.6, d))
    mats = orc.fastfood_matrices(nb, d, 3)
    d2, k, n = orc.fastfood_dims(nb, d)
    assert d2 in wc.D2S and len(cols) == 256 and cols.max() < 4 * n
    seams = {c for blk in range(4) for c in (blk * n, (blk + 1) * n - 1)} | {blk * n + e for blk in (1, 2, 3) for e in (-1, 0)}
    assert seams | {d2 - 1, d2} <= set(cols.tolist())
    assert normwise(orc.fastfood_gm_transform(X, *mats, mean, ard)[:, cols], g["Phi_" + tag]) < 1e-12
    assert set(g.keys()) >= {"X_" + tag, "mean_" + tag, "ls_ard_" + tag, "cols_" + tag, "Phi_" + tag}


def test_cases_reach_every_reachable_instance():
    """Routed by `instance`: every register count in the vector and the scalar variant, in both arithmetics; every d2 with
    d = d2 / 2 + 1, d2 - 1 and d2, k = 1, 3, 4, 5 and N = 1, 2, 7, 37; each alignment rule flips VEC on its own; all eight dtype
    combinations; host-buffer and device-resident calls at every d2."""
    hit = {}
    for c in gc.ALL_CASES + gc.RP_CASES:
        hit.setdefault((c.compute, gc.case_instance(c)), c.label)
    want = gc.reachable_instances()
    for key in sorted(want, key=str):
        print("%-4s %-40s %s" % (key[0], gc.ident(key[1]), hit.get(key, "NOT HIT")))
    assert want <= set(hit), sorted(str(k) for k in want - set(hit))
    assert {gc.ident(k[1]) for k in hit} == set(gc.all_idents())
    assert not set(gc.all_idents()) & set(wc.all_idents())
    for compute in ("f32", "f64"):
        mine = [c for c in gc.GRID if c.compute == compute]
        for d2 in wc.D2S:
            assert {c.d for c in mine if c.d2 == d2} >= {d2 // 2 + 1, d2 - 1, d2}
            assert {c.api for c in gc.ALL_CASES if c.d2 == d2 and c.compute == compute} == {"host", "dev"}
            assert sum(1 for c in gc.RP_CASES if c.d2 == d2 and c.compute == compute and c.N == gc.RP + 1) == 1
        assert {c.k for c in mine} == {1, 3, 4, 5} and {c.N for c in mine} == {1, 2, 7, 37}
        assert {(c.xdt, c.odt) for c in gc.DTYPES if c.compute == compute} == {(a, b) for a in ("f32", "f64") for b in ("f32", "f64")}
    assert all(c.mode == "gm" for c in gc.ALL_CASES + gc.RP_CASES)
    base = dict(compute="f32", d2=512, d=512, k=3, ldx=512, ldo=6144, x_align=0, out_align=0)
    assert gc.instance(**base) == (gc.FAMILY, 8, True, None)
    for kw in ({"ldx": 513}, {"ldo": 6145}, {"d": 511}, {"x_align": 1}, {"out_align": 1}):
        assert gc.instance(**dict(base, **kw))[2] is False, kw
    assert gc.instance(**dict(base, d2=4096, d=4096))[1] == 64
    flips = {c.label.rsplit("/", 1)[1]: gc.case_instance(c)[2] for c in gc.VARIANTS if c.label.startswith("widegm/dev/f32/d2=512/")}
    assert flips == {"aligned": True, "ldx+1": False, "ldo+1": False, "ldo+4": True, "x+1": False, "out+1": False}, flips


@pytest.mark.parametrize("d2", wc.D2S)
def test_phase_plus_shift_stays_exact(d2):
    """|I| + |M| (bounded by the absolute-value chain plus |X| @ |m|) stays below 2^24 for every case of this block size, |M| <=
    384, the shift is non-zero in every row of the largest shape and the length scales are not all one."""
    for c in gc.ALL_CASES + gc.RP_CASES + gc.ZERO_MEAN_CASES + [gc.HUGE_LS_CASE]:
        if c.d2 != d2:
            continue
        D = gc.case_data(c)
        aM = np.abs(D.X).astype(np.int64) @ np.abs(D.m)
        worst = int((D.A.max(axis=1) + aM).max())
        assert np.array_equal(D.M, D.X.astype(np.int64) @ D.m) and np.abs(D.M).max() <= aM.max() <= gc.M_MAX
        assert (np.abs(D.I).max(axis=1) + np.abs(D.M)).max() <= worst < EXACT["f32"] <= EXACT[c.compute], c.label
        assert set(np.unique(D.m)) <= {-2, -1, 0, 1, 2} and len(np.unique(1.0 / D.ls)) > 1
        assert np.array_equal(D.mean * 0.15915494309189533576888, D.m / 16)
    D = gc.case_data(next(c for c in gc.GRID if c.d2 == d2 and c.N == 37))
    print("d2=%d: max |I| %d, max |M| %d, rows with M != 0: %d of 37" % (d2, np.abs(D.I).max(), np.abs(D.M).max(), (D.M != 0).sum()))
    assert (D.M != 0).sum() >= 30 and len(set(D.M.tolist())) > 10


def test_the_keyword_of_the_basis():
    """FastFoodGM(wide_chain=True): Xdim = 5000 raises naming 4096; (d2, k, n) at Xdim = 2049; the class attribute stays False;
    repr and a pickle round trip carry the keyword, and the default's repr is unchanged."""
    import revrand_amd.basis_functions as bs
    with pytest.raises(ValueError, match="4096"):
        bs.FastFoodGM(nbases=8, Xdim=5000, random_state=0, wide_chain=True)
    b = bs.FastFoodGM(nbases=4097, Xdim=2049, random_state=0, wide_chain=True)
    assert (b.d2, b.k, b.n) == (4096, 2, 8192) and b.get_dim(None) == 4 * 8192
    assert bs.FastFoodGM._wide_chain is False and type(b)._wide_chain is False and b.wide_chain is True
    assert repr(b).endswith(", wide_chain=True)")
    plain = bs.FastFoodGM(nbases=8, Xdim=20, random_state=0)
    assert plain.wide_chain is False and repr(plain).endswith("random_state=0)") and "wide_chain" not in repr(plain)
    b2 = pickle.loads(pickle.dumps(b))
    assert b2.wide_chain is True and repr(b2) == repr(b) and np.array_equal(b2.G, b.G) and "_hip_handle" not in b2.__dict__
    # the keyword survives apply_ind and concatenation; Xdim <= 256 is accepted with it
    s = bs.FastFoodGM(nbases=8, Xdim=300, random_state=0, wide_chain=True, apply_ind=list(range(300)))
    assert s.wide_chain is True and s.apply_ind == list(range(300))
    cat = s + bs.LinearBasis(onescol=True)
    assert cat.bases[0] is s and cat.bases[0].wide_chain is True
    assert bs.FastFoodGM(nbases=8, Xdim=20, random_state=0, wide_chain=True).d2 == 32
    # without the keyword a wide basis can still be made (it has no device route: transform raises on the GPU)
    assert bs.FastFoodGM(nbases=8, Xdim=5000, random_state=0).wide_chain is False


def test_wide_gm_entry_point_has_the_signature_of_the_narrow_one():
    from revrand_amd import _hip
    assert _hip.SIGNATURES["rr_fastfood_create_wide_gm"] == _hip.SIGNATURES["rr_fastfood_create"]
    assert _hip.SIGNATURES["rr_fastfood_create_wide"] == _hip.SIGNATURES["rr_fastfood_create"]
    import os
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "revrand_hip.h")).read()
    assert "int rr_fastfood_create_wide_gm(rr_ctx *ctx, int compute, int d, int d2, int k, const int64_t *B, const double *G," in header
