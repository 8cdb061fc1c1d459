"""Spectral-mixture (FastFoodGM) children of the many-steps-per-launch kernel (rr_glm_svi_create_gm,
``GeneralizedLinearModel(resident_bases="all", fused_bases="all+gm")``) -- without a GPU: the dense restatement the GPU tests
compare against (tests/gm_cases.py) held to the oracle's chain, which tests/test_oracle_golden.py pins to the reference's
recorded values; the mixed case's own sanity; the keyword's validation; the ctypes signatures."""
import ctypes

import numpy as np
import pytest

import gm_cases as gc
import revrand_oracle as orc
from conftest import normwise


@pytest.mark.parametrize("case", [(3, 8, 4), (1, 10, 3)])
def test_dense_restatement_agrees_with_the_oracle_s_chain(golden, case):
    """tests/golden/fastfood_gm.npz d3_nb8 and d1_nb10: V = the chain applied to I_d (it is linear in x)"""
    d, nb, seed = case
    g = golden("fastfood_gm")
    k = "d%d_nb%d" % (d, nb)
    B, G, PI, S = orc.fastfood_matrices(nb, d, seed)
    X, mean, ls = g[k + "_X"], g[k + "_mean"], g[k + "_ls"]
    V = orc.fastfood_VX(np.eye(d), B, G, PI, S)
    assert V.shape[0] == d
    Phi = gc.gm_transform(X, V, mean, ls)
    dM, dL = gc.gm_grad(X, V, mean, ls)
    rM, rL = orc.fastfood_gm_grad(X, B, G, PI, S, mean, ls)
    assert dM.shape == rM.shape and dL.shape == rL.shape and dM.ndim == (2 if d == 1 else 3)
    e = (normwise(Phi, orc.fastfood_gm_transform(X, B, G, PI, S, mean, ls)), normwise(dM, rM), normwise(dL, rL))
    print("dense restatement vs oracle chain %s: Phi %.2e dmean %.2e dlen %.2e" % ((k,) + e))
    assert all(v < 1e-12 for v in e), e
    assert normwise(Phi, g[k + "_Phi"]) < 1e-12   # ... and with the reference's recorded features directly


def test_mixed_case_has_finite_oracle_values_and_a_gradient_in_every_slot():
    c = gc.Mixed()
    assert [s.stop - s.start for s in c.slices] == [6, 32, 12, 20] and c.F == 70 and c.M * (5 + 3 + 5 + 1) == 280
    assert c.x0.size == 2 * c.F * c.K + 4 + 1 + c.n_ls and c.n_ls == 13
    assert c.mean1[1] == 0.0 and c.mean1[2] < 0 and c.mean2[0] < 0      # a zero and negative means
    assert not c.positive[c.mean_slots].any() and c.positive[c.len_slots].all()
    for t in range(4):
        obj, grad = c.elbo(c.x0, c.idx[t], c.e[t])
        assert np.isfinite(obj) and np.all(np.isfinite(grad)) and np.all(grad[-13:] != 0)
        assert len(set(c.idx[t].tolist())) == c.M


def test_all_gm_without_resident_bases_all_is_refused_at_fit():
    import revrand_amd.basis_functions as bs
    from revrand_amd import glm
    from revrand_amd import likelihoods as lk
    rs = np.random.RandomState(0)
    X, y = rs.randn(20, 2), rs.randn(20)
    for kw in ({}, {"resident_bases": "fourier"}):
        model = glm.GeneralizedLinearModel(lk.Gaussian(), bs.LinearBasis(), fused_bases="all+gm", **kw)
        with pytest.raises(ValueError) as e:
            model.fit(X, y)
        assert "fused_bases" in str(e.value) and "resident_bases" in str(e.value) and "all+gm" in str(e.value)
    model = glm.GeneralizedLinearModel(lk.Gaussian(), bs.LinearBasis(), resident_bases="all", fused_bases="all+gmm")
    with pytest.raises(ValueError, match="fused_bases"):
        model.fit(X, y)


def test_ctypes_signatures_of_the_new_entry_points():
    import inspect
    from revrand_amd import _hip
    res, args = _hip.SIGNATURES["rr_glm_svi_supported_gm"]
    assert res is ctypes.c_int and args == [ctypes.c_int] * 8
    res, args = _hip.SIGNATURES["rr_glm_svi_create_gm"]
    assert res is ctypes.c_int and args == _hip.SIGNATURES["rr_glm_svi_create_all"][1] and len(args) == 25
    res, args = _hip.SIGNATURES["rr_featmat_put_gm"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    p = inspect.signature(_hip.FusedSvi.__init__).parameters
    assert p["gm_children"].default is False and p["all_children"].default is False
    assert callable(_hip.svi_supported_gm) and callable(_hip.FeatureMatrix.put_gm)


@pytest.mark.parametrize("d,d2,chain_ok,want", [(3, 4, False, "dense"), (8, 8, False, "dense"), (12, 16, True, "chain"),
                                                (200, 256, True, "chain"), (300, 512, False, None)])
def test_dense_child_only_below_the_chain_s_block_sizes(monkeypatch, d, d2, chain_ok, want):
    """`gm_chain_ok` is 16 <= d2 <= 256: false BELOW (Xdim <= 8: the dense handle serves it under the opt-in) and ABOVE
    (Xdim > 256: beyond the dense handle's 128 columns too -- no child, with or without the opt-in, so the fit routes as under
    fused_bases="all")."""
    import types
    import revrand_amd.basis_functions as bs
    made = []
    monkeypatch.setattr(bs, "_ResidentFastFoodGM", lambda basis, X, dense=False: made.append(dense) or ("child", dense))
    b = bs.FastFoodGM(nbases=8, Xdim=d, random_state=0)
    b._handles = lambda: (types.SimpleNamespace(d2=d2, gm_chain_ok=chain_ok), None)
    X = np.zeros((4, d))
    plain, opted = b._resident_child(X), b._resident_child(X, dense_gm=True)
    assert plain == (("child", False) if want == "chain" else None)
    assert opted == {"dense": ("child", True), "chain": ("child", False), None: None}[want]
    feats = bs.MinibatchFeatures(b)
    assert feats.make_resident(X, "all") is (want == "chain")
    assert feats.make_resident(X, "all", dense_gm=True) is (want is not None)
    assert feats.make_resident(X, "all+gm") is (want == "chain")   # (not a value of this keyword: nothing opts in through it)
