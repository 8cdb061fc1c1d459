"""`GeneralizedLinearModel(resident_bases=...)` and the child record of the resident SVI loop (rr_glm_sgd_child), without a GPU:
the keyword's validation and its round trip through the scikit-learn protocol, and the ABI of the record that gained `order`
(include/revrand_hip.h: the field sits in the struct's former tail padding, so its size stays 32 bytes)."""
import ctypes
import pickle

import numpy as np
import pytest


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd import glm
    return bs, lk, glm


def test_unknown_resident_bases_is_refused_at_fit():
    bs, lk, glm = _imports()
    rs = np.random.RandomState(0)
    X, y = rs.randn(20, 2), rs.randn(20)
    model = glm.GeneralizedLinearModel(lk.Gaussian(), bs.LinearBasis(), resident_bases="bogus")   # (the constructor stores)
    with pytest.raises(ValueError, match="resident_bases"):
        model.fit(X, y)


@pytest.mark.parametrize("cls", ["GeneralizedLinearModel", "GeneralisedLinearModel"])
def test_keyword_round_trips_through_get_params_clone_and_pickle(cls):
    from sklearn.base import clone
    bs, lk, glm = _imports()
    GLM = getattr(glm, cls)
    assert GLM(lk.Gaussian(), bs.LinearBasis()).get_params()["resident_bases"] == "fourier"   # the default: today's routing
    model = GLM(lk.Gaussian(), bs.LinearBasis(), resident_bases="all", random_state=3)
    assert model.get_params()["resident_bases"] == "all"
    assert clone(model).resident_bases == "all"
    assert pickle.loads(pickle.dumps(model)).resident_bases == "all"
    assert model.set_params(resident_bases="fourier").resident_bases == "fourier"


def test_child_record_keeps_its_size_with_order_in_the_tail_padding():
    from revrand_amd import _hip
    assert ctypes.sizeof(_hip.SgdChild) == 32
    assert _hip.SgdChild.order.offset == 28 and _hip.SgdChild.n_ls.offset == 24
    assert [f[0] for f in _hip.SgdChild._fields_] == ["kind", "basis", "d", "onescol", "n_ls", "order"]
    assert _hip.SGD_CHILD_KINDS == {"rff": 0, "linear": 1, "gm": 2, "centres": 3, "poly": 4}


def test_child_tuples_fill_the_record():
    from revrand_amd import _hip

    class H(object):
        h = ctypes.c_void_p(0x1000)
    k = _hip.SgdChild()
    assert _hip._fill_sgd_child(k, ("centres", H(), 4)) == 4
    assert (k.kind, k.basis, k.d, k.onescol, k.n_ls, k.order) == (3, 0x1000, 0, 0, 4, 0)
    assert _hip._fill_sgd_child(k, ("poly", 3, False, 2)) == 0
    assert (k.kind, k.basis, k.d, k.onescol, k.n_ls, k.order) == (4, None, 3, 0, 0, 2)
    assert _hip._fill_sgd_child(k, ("linear", 5, True)) == 0
    assert (k.kind, k.basis, k.d, k.onescol, k.n_ls, k.order) == (1, None, 5, 1, 0, 0)
    assert _hip._fill_sgd_child(k, ("gm", H(), 6)) == 6 and k.kind == 2
    assert _hip._fill_sgd_child(k, ("rff", H(), 1)) == 1 and k.kind == 0
