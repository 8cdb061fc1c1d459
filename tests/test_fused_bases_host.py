"""`GeneralizedLinearModel(fused_bases=...)` -- which children the many-steps-per-launch kernel of small minibatches
(rr_svi.hip) takes -- without a GPU: the keyword's default, its validation at `fit`, its round trip through the scikit-learn
protocol, and the ctypes signatures of the two entry points behind "all" (rr_glm_svi_create_all, rr_glm_svi_supported_all)."""
import ctypes
import pickle

import numpy as np
import pytest


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd import glm
    return bs, lk, glm


def _xy():
    rs = np.random.RandomState(0)
    return rs.randn(20, 2), rs.randn(20)


@pytest.mark.parametrize("cls", ["GeneralizedLinearModel", "GeneralisedLinearModel"])
def test_default_is_fourier(cls):
    bs, lk, glm = _imports()
    model = getattr(glm, cls)(lk.Gaussian(), bs.LinearBasis())
    assert model.fused_bases == "fourier" and model.get_params()["fused_bases"] == "fourier"   # the default: today's routing


@pytest.mark.parametrize("cls", ["GeneralizedLinearModel", "GeneralisedLinearModel"])
def test_keyword_round_trips_through_get_params_clone_pickle_and_set_params(cls):
    from sklearn.base import clone
    bs, lk, glm = _imports()
    GLM = getattr(glm, cls)
    model = GLM(lk.Gaussian(), bs.LinearBasis(), resident_bases="all", fused_bases="all", random_state=3)
    assert model.get_params()["fused_bases"] == "all"
    assert clone(model).fused_bases == "all"
    assert pickle.loads(pickle.dumps(model)).fused_bases == "all"
    assert model.set_params(fused_bases="fourier").fused_bases == "fourier"


def test_a_pickle_from_before_the_keyword_reads_as_fourier():
    """`fit` reads the keyword with getattr(..., "fourier"): an estimator without the attribute validates and routes as before."""
    bs, lk, glm = _imports()
    model = glm.GeneralizedLinearModel(lk.Gaussian(), bs.LinearBasis(), resident_bases="bogus")
    del model.__dict__["fused_bases"]
    X, y = _xy()
    with pytest.raises(ValueError, match="resident_bases"):   # (got past the fused_bases checks' getattr, stopped by the next one)
        model.fit(X, y)


def test_unknown_fused_bases_is_refused_at_fit():
    bs, lk, glm = _imports()
    X, y = _xy()
    model = glm.GeneralizedLinearModel(lk.Gaussian(), bs.LinearBasis(), resident_bases="all", fused_bases="bogus")   # (the constructor stores)
    with pytest.raises(ValueError, match="fused_bases"):
        model.fit(X, y)


@pytest.mark.parametrize("resident", ["fourier", None])
def test_all_without_resident_bases_all_is_refused_at_fit(resident):
    bs, lk, glm = _imports()
    X, y = _xy()
    kw = {} if resident is None else {"resident_bases": resident}
    model = glm.GeneralizedLinearModel(lk.Gaussian(), bs.LinearBasis(), fused_bases="all", **kw)
    with pytest.raises(ValueError) as e:
        model.fit(X, y)
    assert "fused_bases" in str(e.value) and "resident_bases" in str(e.value)   # names both keywords


def test_ctypes_signatures_of_the_new_entry_points():
    from revrand_amd import _hip
    res, args = _hip.SIGNATURES["rr_glm_svi_supported_all"]
    assert res is ctypes.c_int and args == [ctypes.c_int] * 8   # rr_glm_svi_supported's seven + table_entries
    res, args = _hip.SIGNATURES["rr_glm_svi_create_all"]
    assert res is ctypes.c_int and args == _hip.SIGNATURES["rr_glm_svi_create"][1]   # "same arguments"
    assert len(args) == 25 and args[-1] == ctypes.POINTER(ctypes.c_void_p)
    import inspect
    assert inspect.signature(_hip.FusedSvi.__init__).parameters["all_children"].default is False
    assert callable(_hip.svi_supported_all)
