"""`GeneralizedLinearModel(predict_engine=...)` without a GPU: the keyword, the boundary of the two entry points behind it
and the likelihoods' `predictive_spec` (what runs on the device is in test_gpu_glm_predictive.py)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _header():
    src = open(os.path.join(ROOT, "include", "revrand_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_constants(prefix):
    return {k: int(v) for k, v in re.findall(r"#define\s+(%s[A-Z_]+)\s+(\d+)" % prefix, _header())}


def _fitted(glm, D=3):
    glm.weights_, glm.covariance_ = np.zeros((D, glm.K)), np.ones((D, glm.K))
    glm.regularizer_, glm.like_hypers_, glm.basis_hypers_ = 1.0, [], []
    return glm


def test_both_entry_points_are_declared_and_in_the_ctypes_table():
    from revrand_amd import _hip
    src = _header()
    for name in ("rr_featmat_predictive", "rr_lik_eval"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["rr_featmat_predictive"][1]) == 11
    assert len(_hip.SIGNATURES["rr_lik_eval"][1]) == 9
    pred, ev = _header_constants("RR_PRED_"), _header_constants("RR_EVAL_")
    assert {k: pred["RR_PRED_" + k.upper()] for k in _hip.PREDICTIVE_IDS} == _hip.PREDICTIVE_IDS
    assert {k: ev["RR_EVAL_" + k.upper()] for k in _hip.LIK_EVAL_IDS} == _hip.LIK_EVAL_IDS
    assert len(pred) == 4 and len(ev) == 3


def test_unknown_predict_engine_is_refused():
    from revrand_amd.glm import GeneralizedLinearModel
    glm = _fitted(GeneralizedLinearModel(K=2, predict_engine="nope"))
    X = np.zeros((4, 2))
    for call in (lambda: glm.predict(X), lambda: glm.predict_moments(X), lambda: glm.predict_cdf(X, 0.0),
                 lambda: glm.predict_logpdf(X, np.zeros(4)), lambda: glm.predict_interval(X, 0.9),
                 lambda: glm.fit(X, np.zeros(4))):
        with pytest.raises(ValueError, match="predict_engine"):
            call()


def test_clone_and_get_params_round_trip_the_keyword():
    from sklearn.base import clone
    from revrand_amd.glm import GeneralizedLinearModel
    assert GeneralizedLinearModel().get_params()["predict_engine"] == "host"
    glm = GeneralizedLinearModel(K=3, predict_engine="device")
    assert glm.get_params()["predict_engine"] == "device"
    twin = clone(glm)
    assert twin.predict_engine == "device" and twin.K == 3
    assert clone(glm.set_params(predict_engine="host")).predict_engine == "host"
    assert "predict_engine" not in repr(glm)   # (the reference's repr, unchanged)


def test_a_likelihood_without_predictive_spec_is_a_type_error_under_the_device_engine():
    from revrand_amd.glm import GeneralizedLinearModel
    from revrand_amd.btypes import Parameter

    class Dummy(object):
        params = Parameter()

        def Ey(self, f):
            return f

        def loglike(self, y, f):
            return -(y - f) ** 2

        def cdf(self, y, f):
            return (y > f).astype(float)

    X = np.zeros((4, 2))
    glm = _fitted(GeneralizedLinearModel(Dummy(), K=2, predict_engine="device", random_state=3))
    state = glm.random_.get_state()
    for call in (lambda: glm.predict(X), lambda: glm.predict_moments(X), lambda: glm.predict_cdf(X, 0.0),
                 lambda: glm.predict_logpdf(X, np.zeros(4)), lambda: glm.predict_interval(X, 0.9)):
        with pytest.raises(TypeError, match="predictive_spec"):
            call()
    # refused before anything was drawn, assembled or uploaded
    assert all(np.array_equal(a, b) for a, b in zip(state, glm.random_.get_state()))
    assert "_serve_feats" not in glm.__dict__


def test_predictive_spec_returns_the_ids_of_the_header():
    from revrand_amd import likelihoods as lk
    ids = _header_constants("RR_LIK_")
    n = np.array([3.0, 5.0, 8.0])
    assert lk.Bernoulli().predictive_spec([], [], 3) == (ids["RR_LIK_BERNOULLI"], 0.0, None)
    lid, par, rowarg = lk.Binomial().predictive_spec([], [n], 3)
    assert (lid, par) == (ids["RR_LIK_BINOMIAL"], 0.0) and np.array_equal(rowarg, n) and rowarg.dtype == np.float64
    assert lk.Gaussian().predictive_spec([0.3], [], 3) == (ids["RR_LIK_GAUSSIAN"], 0.3, None)
    assert lk.Poisson("exp").predictive_spec([], [], 3) == (ids["RR_LIK_POISSON_EXP"], 0.0, None)
    assert lk.Poisson("softplus").predictive_spec([], [], 3) == (ids["RR_LIK_POISSON_SOFTPLUS"], 0.0, None)
    with pytest.raises(ValueError):
        lk.Binomial().predictive_spec([], [], 3)   # n is not optional


def test_the_gaussian_spec_validates_its_variance():
    from revrand_amd import likelihoods as lk
    with pytest.raises(ValueError, match="out of bounds"):
        lk.Gaussian().predictive_spec([-0.5], [], 3)
    lik = lk.Gaussian()
    assert lik.predictive_spec([], [], 3)[1] == lik.params.value   # (no hyper-parameter given: the prior's value, as _check_param)
