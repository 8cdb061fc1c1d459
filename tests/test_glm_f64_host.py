"""`GeneralizedLinearModel(dtype="f64")` without a GPU: the row-slab planner of the float64 step's Ed product (rr_glm64_plan,
host only), the keyword, what it refuses before any device call, and the ABI's declarations (what runs on the device is in
test_gpu_glm_f64.py)."""
import itertools
import os
import re

import numpy as np
import pytest

import glm_f64_cases as gc
from conftest import ROOT

NEW_ENTRY_POINTS = ("rr_glm64_plan", "rr_featmat64_glm_step", "rr_featmat64_glm_step_draws", "rr_featmat64_glm_rff",
                    "rr_featmat64_glm_centres", "rr_featmat64_glm_edphi", "rr_featmat64_project")


def _sweep():
    rows = (1, 16, 127, 128, 129, 300, 384, 1000, 2048, 4224, 10 ** 4, 65536, 10 ** 6)
    Fs = (1, 64, 128, 129, 200, 1000, 2048, 8192)
    KLs = (1, 24, 128, 129, 150, 500, 4096)
    cus = (1, 8, 64, 104, 256, 304)
    return itertools.product(rows, Fs, KLs, cus)


def test_plan_properties_over_a_sweep():
    from revrand_amd import _hip
    n = 0
    for rows, F, KL, cu in _sweep():
        slabs, length, tiles, rp = _hip.glm64_plan(rows, F, KL, cu)
        where = (rows, F, KL, cu, slabs, length, tiles, rp)
        assert rp == -(-rows // 128) * 128 and tiles == (-(-KL // 128)) * (-(-F // 128)), where
        assert slabs >= 1, where
        assert length >= 16 and length % 16 == 0, where
        assert slabs * length >= rp, where
        assert (slabs - 1) * length < rp, where          # the last slab is not empty
        assert slabs <= rp // 128, where
        if tiles >= 2 * cu:
            assert slabs == 1, where
        if tiles < cu:                                    # tiles x slabs reaches the CU count whenever rows_pad / 128 allows
            assert tiles * slabs >= cu or slabs == rp // 128, where
        assert (slabs, length, tiles, rp) == gc.plan_reference(rows, F, KL, cu), where
        n += 1
    assert n > 4000


def test_plan_of_the_benchmarks_glm_shape_has_several_slabs():
    """bench.py config 5: 65 536 rows, F = 2048, K L = 500 on 256 CUs -- 4 x 16 = 64 tiles with a k-loop of 65 536."""
    from revrand_amd import _hip
    slabs, length, tiles, rp = _hip.glm64_plan(65536, 2048, 500, 256)
    assert tiles == 64 and rp == 65536
    assert slabs == 4 and length == 16384     # the smallest count with 64 x slabs >= 256
    # the smallest ragged case of the GPU test: 300 rows in three slabs of 128 padded rows (128 + 128 + 44 data rows)
    assert _hip.glm64_plan(300, 200, 150, 1)[:2] == (1, 384)
    assert _hip.glm64_plan(300, 200, 150, 12)[:2] == (3, 128)
    # 33 row tiles in 32 equal slabs of whole 16-row steps would leave the last one empty: 33 slabs of 128
    assert _hip.glm64_plan(4224, 128, 128, 32)[:2] == (33, 128)


def test_plan_refuses_bad_arguments():
    from revrand_amd import _hip
    for bad in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8)):
        with pytest.raises(_hip.HipError):
            _hip.glm64_plan(*bad)


def test_the_new_entry_points_are_declared_and_in_the_ctypes_table():
    from revrand_amd import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "revrand_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["rr_featmat64_glm_step"][1]) == 12
    assert len(_hip.SIGNATURES["rr_featmat64_glm_step_draws"][1]) == 15
    assert "No GLM step" not in open(os.path.join(ROOT, "include", "revrand_hip.h")).read()
    for meth in ("glm_step", "glm_step_draws", "glm_rff", "glm_centres", "glm_edphi", "project"):
        assert callable(getattr(_hip.FeatureMatrix64, meth))


def test_clone_and_get_params_round_trip_the_keyword():
    from sklearn.base import clone
    from revrand_amd.glm import GeneralizedLinearModel
    assert GeneralizedLinearModel().get_params()["dtype"] == "f32"
    glm = GeneralizedLinearModel(K=3, dtype="f64")
    assert glm.get_params()["dtype"] == "f64"
    twin = clone(glm)
    assert twin.dtype == "f64" and twin.K == 3
    assert clone(glm.set_params(dtype="f32")).dtype == "f32"
    assert "dtype" not in repr(glm)   # (the reference's repr, unchanged)
    odd = GeneralizedLinearModel(dtype="f16")
    assert odd.dtype == "f16"          # stored as given; refused at fit


def test_the_features_type_follows_the_keyword():
    from revrand_amd.basis_functions import MinibatchFeatures, MinibatchFeatures64
    from revrand_amd.glm import GeneralizedLinearModel
    assert type(GeneralizedLinearModel()._features()) is MinibatchFeatures
    assert type(GeneralizedLinearModel()._serving()) is MinibatchFeatures
    glm = GeneralizedLinearModel(dtype="f64", resident_bases="all")
    f = glm._features()
    assert type(f) is MinibatchFeatures64 and f.resident_bases == "all"
    assert type(glm._serving()) is MinibatchFeatures64
    assert f.supports_objective_only is True and f.accepts_device_draws is False
    assert f._target_dtype is np.float64 and MinibatchFeatures._target_dtype is np.float32
    with pytest.raises(TypeError):
        f.predictive(None, None, None, None, None)
    with pytest.raises(TypeError):
        f.glm_step_sampled(None, None, 0, 0.0, None, None, 1, 1, 0, 0)
    # the resident SGD loop declines any features type other than the plain one
    glm._resident_fit = True
    assert glm._resident_loop([None] * 5) is None


REFUSED = [dict(dtype="f16"), dict(dtype=None), dict(dtype="f64", sampler="device"), dict(dtype="f64", devices=[0]),
           dict(dtype="f64", distributed=True), dict(dtype="f64", predict_engine="device"), dict(dtype="f64", gram_engine="bf16x3"),
           dict(dtype="f64", gram_engine="bf16x4"), dict(dtype="f64", gram_engine="fp16x3"),
           dict(dtype="f64", resident_bases="all", fused_bases="all"), dict(dtype="f64", resident_bases="all", fused_bases="all+gm")]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join("%s=%s" % it for it in sorted(kw.items(), key=str)))
def test_refused_before_any_device_call(kw, monkeypatch):
    from revrand_amd import _hip
    from revrand_amd.glm import GeneralizedLinearModel

    def no_device(*a, **k):
        raise AssertionError("fit reached the device")
    monkeypatch.setattr(_hip, "get_device", no_device)
    monkeypatch.setattr(_hip, "load_library", no_device)
    glm = GeneralizedLinearModel(K=2, **kw)
    with pytest.raises(ValueError, match="dtype"):
        glm.fit(np.zeros((6, 2)), np.zeros(6))


def test_reference_draws_are_float64_from_the_same_stream():
    """dtype="f64": `_reference_draws` hands back the reference's float64 normals themselves -- the f32 mode's are their
    roundings, in the same order, and both leave the stream in the same state (NumPy's generator: no library needed)."""
    from revrand_amd.glm import GeneralizedLinearModel
    a, b = GeneralizedLinearModel(K=3, nsamples=4, random_state=5, dtype="f64"), GeneralizedLinearModel(K=3, nsamples=4, random_state=5)
    for g in (a, b):
        g._native_draws, g.D_ = False, 7
    ea, eb = a._reference_draws(), b._reference_draws()
    assert ea.dtype == np.float64 and eb.dtype == np.float32 and ea.shape == eb.shape == (12, 7)
    assert np.array_equal(ea, np.random.RandomState(5).randn(12, 7))
    assert np.array_equal(ea.astype(np.float32), eb)
    assert a.random_.randn() == b.random_.randn()
