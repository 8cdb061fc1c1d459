"""RadialBasis, SigmoidalBasis and PolynomialBasis without a GPU: the float64 restatement (tests/centres_cases.py) against
the reference's recorded outputs (tests/golden/centres*.npz), and the host side of the three classes -- constructors,
validation messages, parameter plumbing, concatenation bookkeeping, cloning and pickling."""
import pickle
from functools import reduce
from operator import add

import numpy as np
import pytest

import centres_cases as cc
from conftest import normwise

SHAPES = [(1, 7), (5, 33), (8, 48)]
TAGS = ["iso0.9", "iso1.7", "ard"]


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd.btypes import Bound, Parameter, Positive
    return bs, Bound, Parameter, Positive


def lenscale_of(tag, d):
    return {"iso0.9": 0.9, "iso1.7": 1.7}.get(tag, np.linspace(0.7, 1.6, d))


def golden_arrays(golden, name):
    return golden("centres_sigmoid" if name == "SigmoidalBasis" else "centres")


@pytest.mark.parametrize("name", ["RadialBasis", "SigmoidalBasis"])
@pytest.mark.parametrize("d,M", SHAPES)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_reference(golden, name, d, M, tag):
    g, gb = golden("centres"), golden_arrays(golden, name)
    X, C = g["X_d%d" % d], g["C_d%d" % d]
    assert X.shape == (32, d) and C.shape == (M, d)
    ls = lenscale_of(tag, d)
    Phi, dPhi = gb["%s_d%d_%s_Phi" % (name, d, tag)], gb["%s_d%d_%s_dPhi" % (name, d, tag)]
    assert dPhi.shape == ((32, M) if (tag != "ard" or d == 1) else (32, M, d))
    assert normwise(cc.TRANSFORM[name](X, C, ls), Phi) <= 1e-12
    assert normwise(cc.GRAD[name](X, C, ls), dPhi) <= 1e-12


@pytest.mark.parametrize("tag,order,bias", [("o0", 0, True), ("o3", 3, True), ("o3nb", 3, False)])
def test_polynomial_restatement_and_class_equal_reference(golden, tag, order, bias):
    bs, _, _, _ = _imports()
    g = golden("centres")
    X, Phi = g["poly_X"], g["poly_%s_Phi" % tag]
    assert normwise(cc.poly_transform(X, order, bias), Phi) <= 1e-12
    b = bs.PolynomialBasis(order=order, include_bias=bias)
    P = b.transform(X)
    assert P.dtype == np.float64 and normwise(P, Phi) <= 1e-12
    assert b.grad(X) == [] and b.get_dim(X) == Phi.shape[1]
    # apply_ind slices the columns first
    b2 = bs.PolynomialBasis(order=order, include_bias=bias, apply_ind=[2, 0])
    assert normwise(b2.transform(X), cc.poly_transform(X[:, [2, 0]], order, bias)) <= 1e-12


def test_constructor_defaults_and_repr():
    bs, Bound, Parameter, Positive = _imports()
    C = np.arange(6.).reshape(3, 2)
    for cls in (bs.RadialBasis, bs.SigmoidalBasis):
        b = cls(centres=C)
        assert (b.M, b.d) == (3, 2) and b.C is C and b.dtype == "f32" and b.apply_ind is None
        assert b.params.shape == () and b.params.is_random and isinstance(b.params.bounds, Positive)
        assert b.regularizer.shape == () and isinstance(b.regularizer.bounds, Positive)
        assert b.get_dim(np.zeros((4, 2))) == 3
        assert repr(b) == "{}(centres={}, lenscale={}, regularizer={})".format(cls.__name__, C, b.params, b.regularizer)
        ard = cls(centres=C, lenscale=Parameter(np.array([1., 2.]), Positive()), regularizer=Parameter(2., Positive()),
                  dtype="f64", apply_ind=[0, 2])
        assert ard.params.shape == (2,) and ard.regularizer.value == 2. and ard.dtype == "f64" and ard.apply_ind == [0, 2]
        with pytest.raises(ValueError, match="dtype must be"):
            cls(centres=C, dtype="f16")
    assert issubclass(bs.SigmoidalBasis, bs.RadialBasis)
    p = bs.PolynomialBasis(order=2)
    assert p.order == 2 and p.include_bias is True and not p.params.has_value
    assert repr(p) == "PolynomialBasis(order=2, include_bias=True, regularizer={})".format(p.regularizer)
    import revrand_amd
    assert revrand_amd.RadialBasis is bs.RadialBasis and revrand_amd.PolynomialBasis is bs.PolynomialBasis


def test_validation_messages():
    bs, Bound, Parameter, Positive = _imports()
    C = np.zeros((4, 3))
    for cls in (bs.RadialBasis, bs.SigmoidalBasis):
        with pytest.raises(ValueError, match="Parameter dimension doesn't agree with X dimensions!"):
            cls(centres=C, lenscale=Parameter(np.ones(2), Positive()))
        b = cls(centres=C)
        # both checks come before any device call
        with pytest.raises(ValueError, match="Dimensions of data inconsistent!"):
            b.transform(np.zeros((2, 4)))
        with pytest.raises(ValueError, match="Dimensions of data inconsistent!"):
            b.grad(np.zeros((2, 2)), 1.)
        with pytest.raises(ValueError, match="Dimension of input parameter is inconsistent!"):
            b.transform(np.zeros((2, 3)), np.ones(2))
        with pytest.raises(ValueError, match="Regularizer parameters have to be scalar!"):
            cls(centres=C, regularizer=Parameter(np.ones(2), Positive()))
        with pytest.raises(ValueError, match="Regularizer has to be bounded below by 0!"):
            cls(centres=C, regularizer=Parameter(1., Bound(-1., 2.)))
    with pytest.raises(ValueError, match="Polynomial order must be positive"):
        bs.PolynomialBasis(order=-1)
    with pytest.raises(ValueError, match="Regularizer parameters have to be scalar!"):
        bs.PolynomialBasis(order=1, regularizer=Parameter(np.ones(2), Positive()))


def _cat15(bs, Bound, Parameter, Positive, X, nC=10):
    d = X.shape[1]

    def ard():
        return Parameter(np.ones(d), Positive())
    return [bs.BiasBasis(), bs.LinearBasis(onescol=True), bs.PolynomialBasis(order=2),
            bs.RadialBasis(centres=X[:nC, :]), bs.RadialBasis(centres=X[:nC, :], lenscale=ard()),
            bs.SigmoidalBasis(centres=X[:nC, :]), bs.SigmoidalBasis(centres=X[:nC, :], lenscale=ard()),
            bs.RandomRBF(Xdim=d, nbases=10), bs.RandomRBF(Xdim=d, nbases=10, lenscale=ard()),
            bs.OrthogonalRBF(Xdim=d, nbases=10), bs.OrthogonalRBF(Xdim=d, nbases=10, lenscale=ard()),
            bs.FastFoodRBF(Xdim=d, nbases=10), bs.FastFoodRBF(Xdim=d, nbases=10, lenscale=ard()),
            bs.FastFoodGM(Xdim=d, nbases=10),
            bs.FastFoodGM(Xdim=d, nbases=10, mean=Parameter(np.zeros(d), Bound()), lenscale=ard())]


def test_concatenation_structure_equals_reference(golden):
    """The 15-way concatenation of the reference's own basis test: widths, regulariser slices and parameter routing."""
    bs, Bound, Parameter, Positive = _imports()
    g = golden("centres")
    X = g["cat15_X"]
    bases = _cat15(bs, Bound, Parameter, Positive, X)
    cat = reduce(add, bases)
    assert [int(b.get_dim(X)) for b in bases] == list(g["cat15_dims"])
    assert int(cat.get_dim(X)) == int(g["cat15_get_dim"])
    diag, slices = cat.regularizer_diagonal(X, *g["cat15_regs"])
    assert np.array_equal(diag, g["cat15_regdiag"])
    assert [[s.start, s.stop] for s in slices] == g["cat15_slices"].tolist()
    assert len(cat.regularizer) == 15
    sizes = [(-1 if p.shape == () else int(p.shape[0])) for p in cat.params]
    assert sizes == list(g["cat15_param_sizes"])
    # positional routing: every basis takes as many hyper-parameters as it has parameters, for transform and grad alike
    for b in bases[2:7]:
        npar = 0 if isinstance(b, bs.PolynomialBasis) else 1
        assert bs.count_args(b.transform) - 1 == npar and bs.count_args(b.grad) - 1 == npar
    # host-only children concatenate without a device
    host = bs.PolynomialBasis(order=3, include_bias=False) + bs.LinearBasis() + bs.BiasBasis()
    want = np.hstack((cc.poly_transform(X, 3, False), np.ones((len(X), 1)), X, np.ones((len(X), 1))))
    assert np.array_equal(host.transform(X), want) and list(host.grad(X)) == []


def test_clone_and_pickle_drop_device_handles():
    from sklearn.base import clone
    bs, Bound, Parameter, Positive = _imports()
    from revrand_amd.slm import StandardLinearModel
    C = np.random.RandomState(0).randn(5, 2)
    for basis in (bs.RadialBasis(centres=C), bs.SigmoidalBasis(centres=C, lenscale=Parameter(np.ones(2), Positive())),
                  bs.PolynomialBasis(order=2), bs.RadialBasis(centres=C) + bs.PolynomialBasis(order=2) + bs.LinearBasis()):
        first = basis.bases[0] if hasattr(basis, "bases") else basis
        if hasattr(first, "C"):
            first.__dict__["_hip_handle"] = {("pid", 0): (lambda: None)}  # stands for a device handle: cannot be pickled
        est = StandardLinearModel(basis=basis, nstarts=0)
        for copy in (clone(est), pickle.loads(pickle.dumps(est))):
            got = copy.basis.bases[0] if hasattr(copy.basis, "bases") else copy.basis
            assert type(got) is type(first) and got is not first
            assert "_hip_handle" not in got.__dict__
            if hasattr(first, "C"):
                assert np.array_equal(got.C, C) and got.params.shape == first.params.shape
            else:
                assert (got.order, got.include_bias) == (2, True)
            assert repr(copy.basis) == repr(basis)
