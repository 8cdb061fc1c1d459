"""CPU checks behind tests/test_gpu_fastfood_wide.py: the case list reaches every instance of the wide chain kernel, the
integer data stays exact, the dyadic phases hold at the wide block sizes, the recorded reference agrees with the oracle, and
the new entry point's signature is the old one's."""
import numpy as np
import pytest

import revrand_oracle as orc
from conftest import load_golden, normwise

import fastfood_wide_cases as wc
from test_gpu_fastfood_exact import EXACT, dyadic_S, hadamard_pm1, int_chain

GOLDEN_SHAPES = [(300, 600, 4), (1000, 1500, 3), (2049, 4097, 2), (4096, 4096, 2)]


def test_cases_reach_every_reachable_instance():
    """Routed by `instance`: every register count in the vector and the scalar variant, in both modes and both arithmetics;
    every d2 with d = d2 / 2 + 1, d2 - 1 and d2, k = 1, 3, 4, 5 and N = 1, 2, 7, 37; each alignment rule flips VEC on its own;
    all eight dtype combinations."""
    hit = {}
    for c in wc.ALL_CASES + wc.RP_CASES + [wc.SEAM_CASE]:
        hit.setdefault((c.compute, wc.case_instance(c), c.mode), c.label)
    want = wc.reachable_instances()
    for key in sorted(want, key=str):
        print("%-4s %-40s %s" % (key[0], wc.ident(*key[1:]), hit.get(key, "NOT HIT")))
    assert want <= set(hit), sorted(str(k) for k in want - set(hit))
    assert {wc.ident(*k[1:]) for k in hit} == set(wc.all_idents())
    for compute in ("f32", "f64"):
        mine = [c for c in wc.GRID if c.compute == compute]
        for d2 in wc.D2S:
            assert {c.d for c in mine if c.d2 == d2} >= {d2 // 2 + 1, d2 - 1, d2}
            assert {c.mode for c in mine if c.d2 == d2} == {"vx", "phi"}
            assert {c.api for c in wc.ALL_CASES if c.d2 == d2 and c.compute == compute} == {"host", "dev"}
        assert {c.k for c in mine} == {1, 3, 4, 5} and {c.N for c in mine} == {1, 2, 7, 37}
        assert {(c.xdt, c.odt) for c in wc.DTYPES if c.compute == compute} == {(a, b) for a in ("f32", "f64") for b in ("f32", "f64")}
    # each of the five conditions behind VEC decides on its own
    base = dict(compute="f32", d2=512, d=512, k=3, ldx=512, ldo=3072, x_align=0, out_align=0, mode="phi")
    assert wc.instance(**base) == (wc.FAMILY, 8, True, None)
    for kw in ({"ldx": 513}, {"ldo": 3073}, {"d": 511}, {"x_align": 1}, {"out_align": 1}):
        assert wc.instance(**dict(base, **kw))[2] is False, kw
    assert wc.instance(**dict(base, ldo=3076))[2] and wc.instance(**dict(base, d=260))[2]
    assert wc.instance(**dict(base, compute="f64", x_align=2))[2] and not wc.instance(**dict(base, compute="f64", out_align=1))[2]
    assert wc.instance(**dict(base, d2=4096, d=4096))[1] == 64
    flips = {c.label.rsplit("/", 1)[1]: wc.case_instance(c)[2] for c in wc.VARIANTS if c.label.startswith("wide/dev/f32/d2=512/")}
    assert flips == {"aligned": True, "ldx+1": False, "ldo+1": False, "ldo+4": True, "x+1": False, "out+1": False}, flips
    with pytest.raises(ValueError):
        wc.instance("f32", 512, 300, 3, 300, 6144, 0, 0, "gm")


@pytest.mark.parametrize("d2", wc.D2S)
def test_integer_data_is_exact_and_touches_the_seams(d2):
    """Per shape: at most 64 non-zeros per row, sum |x / l| <= 768, the absolute-value chain below 2^24 (asserted again per case
    when it runs); column 0, column d - 1 and both sides of every 256-element boundary non-zero in every row; lane-boundary pairs
    in every row, different ones from row to row."""
    for d in (d2 // 2 + 1, d2 - 1, d2):
        F = wc.shape_data(d2, d)
        nnz = (F.X != 0).sum(axis=1)
        assert nnz.max() <= wc.NNZ and nnz.min() >= 34
        assert np.abs(F.X).max() <= 3 and set(np.unique(F.inv_ls)) <= {1, 2, 4}
        assert (np.abs(F.X) * F.inv_ls).sum(axis=1).max() <= 768
        print("d2=%d d=%d: max |I| %.3g, bound A %.3g (2^24 = %.3g)" % (d2, d, np.abs(F.I).max(), F.A.max(), EXACT["f32"]))
        assert F.A.max() <= 768 * 3 * d2 < EXACT["f32"]
        must = [0, d - 1] + [c for b in range(256, d, 256) for c in (b - 1, b)]
        assert np.all(F.X[:, must] != 0)
        pairs = [{b for b in range(2, d, 2) if row[b - 1] and row[b]} for row in F.X]
        assert min(len(p) for p in pairs) >= 16
        assert any(b % 4 == 0 for b in pairs[0]) and any(b % 4 == 2 for b in pairs[0])
        n_rows = F.X.shape[0]
        assert n_rows == wc.shape_rows(d2, d) and len({r.tobytes() for r in F.I}) == n_rows  # every row its own pattern
        if d == d2:
            # over the rows of this shape both sides of EVERY lane boundary (every multiple of 2: float64's; every multiple of
            # 4: float32's) are non-zero in some row, and a case runs all of these rows
            assert set().union(*pairs) == set(range(2, d, 2))
            assert any(c.d2 == d2 and c.d == d and c.N == n_rows and c.compute == "f32" for c in wc.ALL_CASES)
            assert any(c.d2 == d2 and c.d == d and c.N == n_rows and c.compute == "f64" for c in wc.ALL_CASES)
        else:
            assert len(set().union(*pairs)) >= min(300, d // 2 - 40)  # (the rows carry different boundaries)


def test_dyadic_phases_hold_at_the_wide_block_sizes():
    for d2 in wc.D2S:
        S, srev = dyadic_S(d2)
        assert abs(srev - 2.0 ** -4) < 1e-16 and np.float32(srev) == np.float32(2.0 ** -4)
        norm = float(d2) ** -1.5
        assert (np.frexp(norm)[0] == 0.5) == (d2 in wc.POW2_NORM)


def test_int_chain_agrees_with_the_oracle_at_512():
    """int_chain * S * d2^-1.5 equals oracle.fastfood_VX on the sparse integer data, and the float64-BLAS route (used from
    d2 = 2048) equals the int64 one."""
    F = wc.shape_data(512, 511)
    I2, A2 = int_chain(F.X, F.inv_ls, F.B, F.G, F.PI, blas=True)
    assert np.array_equal(F.I, I2) and np.array_equal(F.A, A2)
    ref = orc.fastfood_VX(F.X * F.inv_ls.astype(np.float64), F.B, F.G.astype(np.float64), F.PI, F.S_int)
    mine = F.I * np.tile(F.S_int.ravel(), (wc.NMAX, 1)) * 512.0 ** -1.5
    assert F.X.shape == (wc.NMAX, 511)
    assert np.abs(mine - ref).max() <= 4e-16 * np.abs(ref).max()
    H = hadamard_pm1(512)
    assert np.array_equal(H @ H, 512 * np.eye(512, dtype=np.int64))


def test_chunk_seam_case_crosses_one_seam():
    c = wc.SEAM_CASE
    per_row = c.d * 4 + 2 * c.d2 * c.k * 4
    assert (256 << 20) // per_row == wc.SEAM_ROWS_PER_CHUNK < c.N < 2 * wc.SEAM_ROWS_PER_CHUNK
    # the chunk arithmetic of ff_host_call at the widest row this handle kind can have here, in size_t / int64
    assert wc.SEAM_ROWS_PER_CHUNK * 2 * c.d2 * c.k * 4 < 2 ** 63 and c.N * 2 * c.d2 * c.k < 2 ** 31


@pytest.mark.parametrize("shape", GOLDEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_golden_file_against_the_oracle(shape):
    """tests/golden/fastfood_wide.npz (the reference's outputs, tools/make_fastfood_wide_golden.py) against the oracle on the
    stored inputs, at the stored columns: 1e-12 normwise."""
    d, nb, N = shape
    g = load_golden("fastfood_wide")
    tag = "d%d" % d
    X = g["X_" + tag].astype(np.float64)
    assert X.shape == (N, d) and g["X_" + tag].dtype == np.float32
    cols, ard, iso = g["cols_" + tag], g["ls_ard_" + tag], float(g["ls_iso"])
    mats = orc.fastfood_matrices(nb, d, 3)
    d2, k, n = orc.fastfood_dims(nb, d)
    assert d2 in wc.D2S and cols.max() < 2 * n and {0, n - 1, n, 2 * n - 1} <= set(cols.tolist())
    assert normwise(orc.fastfood_transform(X, *mats, iso)[:, cols], g["Phi_iso_" + tag]) < 1e-12
    assert normwise(orc.fastfood_transform(X, *mats, ard)[:, cols], g["Phi_ard_" + tag]) < 1e-12
    assert normwise(orc.fastfood_grad(X, *mats, iso)[:, cols], g["dPhi_iso_" + tag]) < 1e-12
    if d == 300:
        gcols = g["gcols_" + tag]
        assert normwise(orc.fastfood_grad(X, *mats, ard)[:, gcols, :], g["dPhi_ard_" + tag]) < 1e-12
    else:
        assert "dPhi_ard_" + tag not in g


def test_wide_entry_point_has_the_signature_of_the_narrow_one():
    from revrand_amd import _hip
    assert _hip.SIGNATURES["rr_fastfood_create_wide"] == _hip.SIGNATURES["rr_fastfood_create"]
    assert _hip.FASTFOOD_MAX_DIM == 4096


def test_basis_classes_say_who_takes_the_wide_handle():
    """FastFoodRBF allows the wide handle, FastFoodGM does not; Xdim > 4096 is refused when the basis is made, naming 4096."""
    import revrand_amd.basis_functions as bs
    assert bs.FastFoodRBF._wide_chain is True and bs.FastFoodGM._wide_chain is False
    with pytest.raises(ValueError, match="4096"):
        bs.FastFoodRBF(nbases=8, Xdim=5000, random_state=0)
    b = bs.FastFoodRBF(nbases=4097, Xdim=2049, random_state=0)
    assert (b.d2, b.k, b.n) == (4096, 2, 8192)
