"""StandardLinearModel(resident_bases=...) without a device: the constructor attribute as scikit-learn sees it, its validation
before any device call, and the C ABI's four float64 centre / polynomial entry points in the header and the ctypes table."""
import os
import pickle
import re

import numpy as np
import pytest

from conftest import ROOT

NEW_ENTRY_POINTS = ["rr_featmat64_put_centres", "rr_featmat64_put_poly", "rr_featmat64_pass2_centres", "rr_featmat64_download"]


def test_default_is_fourier():
    from revrand_amd.slm import StandardLinearModel
    assert StandardLinearModel().get_params()["resident_bases"] == "fourier"


def test_clone_and_pickle_keep_the_value():
    from sklearn.base import clone
    from revrand_amd.slm import StandardLinearModel
    slm = StandardLinearModel(resident_bases="all")
    assert clone(slm).resident_bases == "all"
    assert pickle.loads(pickle.dumps(slm)).resident_bases == "all"
    assert clone(slm).get_params()["resident_bases"] == "all"


def test_bad_value_is_refused_before_the_library_is_touched(monkeypatch):
    from revrand_amd import _hip
    from revrand_amd.slm import StandardLinearModel

    def no_library(*a, **k):
        raise AssertionError("fit reached the device library before validating resident_bases")
    monkeypatch.setattr(_hip, "load_library", no_library)
    monkeypatch.setattr(_hip, "get_device", no_library)
    rs = np.random.RandomState(0)
    with pytest.raises(ValueError, match="resident_bases must be 'fourier' or 'all'"):
        StandardLinearModel(resident_bases="every").fit(rs.randn(10, 2), rs.randn(10))


def test_header_and_ctypes_table_carry_the_new_entry_points():
    from revrand_amd import _hip
    src = open(os.path.join(ROOT, "include", "revrand_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*rr_featmat64\s*\*" % name, src), name
        assert name in _hip.SIGNATURES and _hip.SIGNATURES[name][0] is _hip.ctypes.c_int
        assert len(_hip.SIGNATURES[name][1]) == {"rr_featmat64_put_centres": 8, "rr_featmat64_put_poly": 8,
                                                 "rr_featmat64_pass2_centres": 7, "rr_featmat64_download": 2}[name]
