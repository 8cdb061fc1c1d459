"""The routing of centre bases with more than 128 input columns, without a GPU: `_resident_child` / `_make_child` give a
device child for 129 .. 4096 columns only when asked (`wide=True`), the makers that stand behind ``resident_bases="all"`` ask,
every default call does not, and the limit the Python side routes by is the header's RR_CENTRES_MAX_DIM."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    from revrand_amd.btypes import Parameter, Positive
    return bs, _hip, Parameter, Positive


class _Child(object):
    """Stands for _ResidentCentres: records what it was made with, touches no device."""
    nparams = 1

    def __init__(self, basis, X, dtype=None):
        self.basis, self.shape, self.dtype = basis, X.shape, dtype

    def release(self):
        pass


@pytest.fixture
def stubbed(monkeypatch):
    bs, _hip, Parameter, Positive = _imports()
    monkeypatch.setattr(bs, "_ResidentCentres", _Child)
    return bs


def _basis(bs, cls, d, dtype="f32", M=3):
    return getattr(bs, cls)(centres=np.zeros((M, d)), dtype=dtype)


@pytest.mark.parametrize("cls", ["RadialBasis", "SigmoidalBasis"])
def test_wide_children_only_on_request(stubbed, cls):
    bs = stubbed
    for d in (1, 128):   # narrow inputs: a child under every call, as before
        b, X = _basis(bs, cls, d), np.zeros((2, d))
        assert isinstance(b._resident_child(X), _Child) and isinstance(b._resident_child(X, wide=True), _Child)
    for d in (129, 130, 1000, 4096):
        b, X = _basis(bs, cls, d), np.zeros((2, d))
        assert b._resident_child(X) is None                    # the default call
        assert b._resident_child(X, wide=False) is None
        c = b._resident_child(X, wide=True)
        assert isinstance(c, _Child) and c.shape == (2, d) and c.dtype is None
    b, X = _basis(bs, cls, 4097), np.zeros((2, 4097))
    assert b._resident_child(X) is None and b._resident_child(X, wide=True) is None


def test_wide_children_follow_the_f64_rule(stubbed):
    """The existing `f64_children` rule is unchanged by `wide`: a float64 state takes the basis only on opt-in, an f32 state
    takes f32 bases only."""
    bs = stubbed
    X = np.zeros((2, 130))
    f32, f64 = _basis(bs, "RadialBasis", 130), _basis(bs, "RadialBasis", 130, dtype="f64")
    assert f32._resident_child(X, dtype="f64", wide=True) is None
    c = f32._resident_child(X, dtype="f64", f64_children=True, wide=True)
    assert isinstance(c, _Child) and c.dtype == "f64"
    assert f64._resident_child(X, wide=True) is None
    assert f64._resident_child(X, dtype="f64", f64_children=True) is None   # wide not asked for
    assert isinstance(f64._resident_child(X, dtype="f64", f64_children=True, wide=True), _Child)


def test_polynomial_basis_tolerates_the_keyword(monkeypatch):
    bs, _hip, Parameter, Positive = _imports()
    monkeypatch.setattr(bs, "_ResidentPoly", _Child)
    p = bs.PolynomialBasis(order=2)
    X = np.zeros((2, 130))
    assert isinstance(p._resident_child(X, wide=True), _Child) and isinstance(p._resident_child(X), _Child)


@pytest.fixture
def recorded(monkeypatch):
    """Every `_make_child` call of the centre bases, declined (None): the makers give up before they touch a device."""
    bs, _hip, Parameter, Positive = _imports()
    calls = []

    def spy(self, X, dtype, f64_children=False, **kw):
        calls.append(dict(kw, dtype=dtype, f64_children=f64_children))
        return None
    monkeypatch.setattr(bs.RadialBasis, "_make_child", spy)
    return bs, calls


def test_makers_pass_the_keyword_under_all_only(recorded):
    bs, calls = recorded
    X, y = np.zeros((4, 130)), np.zeros(4)
    radial = _basis(bs, "RadialBasis", 130)
    cat = bs.BasisCat._of([_basis(bs, "SigmoidalBasis", 130)])

    def wide_of(fn):
        del calls[:]
        assert not fn()            # None / False: the spy declined
        assert len(calls) == 1
        return bool(calls[0].get("wide", False))
    assert wide_of(lambda: radial.device_fit_state(X, y, resident_bases="all")) is True
    assert wide_of(lambda: radial.device_fit_state(X, y)) is False
    assert wide_of(lambda: radial.device_fit_state(X, y, resident_bases="fourier")) is False
    assert wide_of(lambda: cat.device_fit_state(X, y, resident_bases="all")) is True
    assert wide_of(lambda: cat.device_fit_state(X, y)) is False
    for basis in (radial, cat):
        assert wide_of(lambda: bs.MinibatchFeatures(basis).make_resident(X, "all")) is True
        assert wide_of(lambda: bs.MinibatchFeatures(basis).make_resident(X, resident_bases="all")) is True
        assert wide_of(lambda: bs.MinibatchFeatures(basis).make_resident(X)) is False
        assert wide_of(lambda: bs.MinibatchFeatures(basis).make_resident(X, "fourier")) is False


def test_estimators_hand_their_option_on(recorded, monkeypatch):
    """GeneralizedLinearModel.fit gives `make_resident` the estimator's resident_bases ("all"), and calls it as it always did
    under the default; StandardLinearModel's `_make_state` hands `device_fit_state` the same option."""
    bs, calls = recorded
    from revrand_amd.glm import GeneralizedLinearModel
    from revrand_amd.slm import StandardLinearModel
    seen = []

    class Stop(Exception):
        pass

    def make_resident(self, *a, **k):
        seen.append((a[1:], k))
        raise Stop()
    monkeypatch.setattr(bs.MinibatchFeatures, "make_resident", make_resident)
    X, y = np.zeros((8, 130)), np.zeros(8)
    for option, want in (("all", (("all",), {})), ("fourier", ((), {}))):
        glm = GeneralizedLinearModel(basis=_basis(bs, "RadialBasis", 130), resident_bases=option, predict_engine="host")
        with pytest.raises(Stop):
            glm.fit(X, y)
        assert seen.pop() == want
        del calls[:]
        slm = StandardLinearModel(basis=_basis(bs, "RadialBasis", 130), resident_bases=option)
        assert slm._make_state(X, y) is None
        assert len(calls) == 1 and bool(calls[0].get("wide", False)) == (option == "all")


def test_the_limit_is_the_header_s():
    bs, _hip, Parameter, Positive = _imports()
    with open(os.path.join(ROOT, "include", "revrand_hip.h")) as f:
        m = re.findall(r"^#define\s+RR_CENTRES_MAX_DIM\s+(\d+)\s*$", f.read(), flags=re.M)
    assert len(m) == 1 and int(m[0]) == _hip.CENTRES_MAX_DIM == 4096
    assert _hip.CENTRES_NARROW_DIM == 128
