"""The host side of spectral-mixture (FastFoodGM) children in the wide small-minibatch loop (rr_glm_sviwgm_*, rr_svi_wide.hip;
GeneralizedLinearModel(fused_bases="all+gm", wide_fused=True)): the planner's GM items, the LDS budget, the range check, the
refusals that stay and the keyword validation.  None of it needs a device."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

MIXED = [("linear", 5, True), ("gm", 8, 3), ("rff", 6, 5), ("gm", 5, 1)]     # the children of gm_cases.Mixed

_PLAN_CODE = """
import sys, json
sys.path.insert(0, %r)
from revrand_amd import _hip
kids = [("linear", 5, True), ("gm", 8, 3), ("rff", 6, 5), ("gm", 5, 1)]
items, info = _hip.sviw_plan(kids, 3, 20, 20)
print("PLAN " + json.dumps({"items": items, "info": info}))
"""


def _runs(items, child):
    return [(j0, cnt) for (c, j0, cnt) in items if c == child]


@pytest.mark.parametrize("env", ["3", "2", None])
def test_plan_tiles_every_spectral_mixture_child(env):
    """RR_SVIW_ITEM is read by the library: each value in a process of its own."""
    e = dict(os.environ)
    e.pop("RR_SVIW_ITEM", None)
    if env is not None:
        e["RR_SVIW_ITEM"] = env
    r = subprocess.run([sys.executable, "-c", _PLAN_CODE % ROOT], capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0 and "PLAN " in r.stdout, r.stderr[-3000:]
    out = json.loads(r.stdout.split("PLAN ", 1)[1])
    items, info = [tuple(i) for i in out["items"]], out["info"]
    assert info["items"] == len(items) and info["lds_bytes"] <= info["lds_budget"] <= 160 * 1024
    gw = info["gm_width"]
    assert gw == int(env) if env is not None else gw >= 8     # unset: the default cap holds either component in one item
    assert [c for (c, _, _) in items] == sorted(c for (c, _, _) in items)      # in concatenation order, none straddles a child
    assert _runs(items, 0) == [(0, 6)]                    # the linear child: one item of all its columns
    for child, n in ((1, 8), (3, 5)):
        nxt = 0
        runs = _runs(items, child)
        for j0, cnt in runs:                              # consecutive runs: no gap, no overlap
            assert j0 == nxt and 1 <= cnt <= gw
            nxt += cnt
        assert nxt == n
        assert all(cnt == gw for _, cnt in runs[:-1])     # all full-width except the last
    if env == "3":
        assert [cnt for _, cnt in _runs(items, 1)] == [3, 3, 2] and [cnt for _, cnt in _runs(items, 3)] == [3, 2]
        assert [cnt for _, cnt in _runs(items, 2)] == [3, 3]
    if env == "2":
        assert _runs(items, 3)[-1] == (4, 1)              # a last item of one frequency
        assert [cnt for _, cnt in _runs(items, 1)] == [2, 2, 2, 2]
    if env is None:
        assert _runs(items, 1) == [(0, 8)] and _runs(items, 3) == [(0, 5)] and _runs(items, 2) == [(0, 6)]


def test_gm_width_follows_the_lds_budget():
    """Xdim = 128, 300 frequencies at the widest K, L and minibatch of the range: the rows (64 x 128) and dfs (128 x 64) alone
    take 128 KiB, so the width shrinks far below the cap and stays >= 1"""
    from revrand_amd import _hip
    items, info = _hip.sviw_plan([("gm", 300, 128)], 32, 128, 64)
    assert 1 <= info["gm_width"] < 32
    assert info["lds_bytes"] <= info["lds_budget"]
    assert sum(cnt for _, _, cnt in items) == 300 and all(cnt <= info["gm_width"] for _, _, cnt in items)
    # next to a random Fourier child each kind keeps a width of its own
    _, both = _hip.sviw_plan([("gm", 300, 4), ("rff", 300, 4)], 10, 50, 10)
    assert both["width"] == 64 and 1 <= both["gm_width"] <= 64 and both["lds_bytes"] <= both["lds_budget"]


def test_other_kinds_are_still_refused():
    from revrand_amd import _hip
    with pytest.raises(ValueError):
        _hip.sviw_plan([("centres", 10, 2)], 4, 10, 10)
    with pytest.raises(ValueError):
        _hip.sviw_plan([("gm", 8, 3), ("poly", 3, True, 2)], 4, 10, 10)
    # the C entry point of the loop without spectral-mixture children refuses the kind as it always did
    lib = _hip.load_library()
    import ctypes
    kind, n, d = (ctypes.c_int * 1)(2), (ctypes.c_int * 1)(8), (ctypes.c_int * 1)(3)
    info = (ctypes.c_int64 * 4)()
    rc = lib.rr_glm_sviw_plan(1, ctypes.cast(kind, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p), ctypes.cast(d, ctypes.c_void_p),
                              4, 10, 10, 0, None, info)
    assert rc != 0
    kind[0] = 3     # a centre child: refused by the new planner too
    info5 = (ctypes.c_int64 * 5)()
    rc = lib.rr_glm_sviwgm_plan(1, ctypes.cast(kind, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p),
                                ctypes.cast(d, ctypes.c_void_p), 4, 10, 10, 0, None, info5)
    assert rc != 0


def test_range_without_gm_columns_is_the_wide_loop_s_own():
    from revrand_amd import _hip
    for F in (24, 512, 2048, 16384, 40000):
        for M in (10, 32, 64, 65):
            for K in (10, 33):
                for (L, nk, dsum, n_ls) in ((50, 1, 21, 21), (6, 3, 12, 5)):
                    assert _hip.sviw_supported_gm(F, K, L, M, nk, dsum, n_ls, 0) == _hip.sviw_supported(F, K, L, M, nk, dsum, n_ls), \
                        (F, M, K, L)


def test_range_with_gm_columns():
    from revrand_amd import _hip
    # four nbases=32 components on Xdim = 4 at the reference's K = 10, 50 samples, 10 rows: the shape the step-per-call loop kept
    assert _hip.sviw_supported_gm(512, 10, 50, 10, 4, 16, 32, 512)
    assert _hip.sviw_supported_gm(70, 3, 20, 20, 4, 14, 13, 52)        # gm_cases.Mixed
    assert _hip.sviw_supported_gm(24 + 129, 2, 5, 7, 2, 256, 256, 24)  # one component on 128 columns: 256 slots
    assert not _hip.sviw_supported_gm(512, 33, 50, 10, 4, 16, 32, 512)     # K = 33
    assert not _hip.sviw_supported_gm(512, 10, 129, 10, 4, 16, 32, 512)    # nsamples = 129
    assert not _hip.sviw_supported_gm(512, 10, 50, 65, 4, 16, 32, 512)     # minibatch = 65
    assert not _hip.sviw_supported_gm(512, 10, 50, 10, 17, 16, 32, 512)    # 17 children
    assert not _hip.sviw_supported_gm(512, 10, 50, 10, 4, 16, 32, 516)     # more GM columns than columns
    assert not _hip.sviw_supported_gm(512, 10, 50, 10, 4, 16, 32, 510)     # not a multiple of four
    assert not _hip.sviw_supported_gm(40000, 10, 50, 10, 4, 16, 32, 512)


def test_new_entry_points_are_declared_exported_and_in_the_ctypes_table():
    from revrand_amd import _hip
    src = open(os.path.join(ROOT, "include", "revrand_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rr_glm_sviwgm_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["rr_glm_sviwgm_create", "rr_glm_sviwgm_plan", "rr_glm_sviwgm_supported"]
    lib = _hip.load_library()
    for name in declared:
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert callable(_hip.sviw_supported_gm)


def test_creator_selection_needs_no_device():
    from revrand_amd import _hip
    w = _hip.WideSvi.__new__(_hip.WideSvi)
    w.lib = _hip.load_library()
    with pytest.raises(ValueError):
        w._creator(True, False)
    with pytest.raises(ValueError):
        w._creator(True, True)
    assert w._creator(False, True) is w.lib.rr_glm_sviwgm_create
    assert w._creator(False, False) is w.lib.rr_glm_sviw_create
    w.h = None


def _glm(**kw):
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.glm import GeneralizedLinearModel
    return GeneralizedLinearModel(lk.Gaussian(), bs.RandomRBF(nbases=6, Xdim=2, random_state=0), maxiter=3, nstarts=0, **kw)


@pytest.mark.parametrize("kw, match", [
    (dict(wide_fused="yes", fused_bases="all+gm", resident_bases="all"), "wide_fused"),
    (dict(wide_fused=True, fused_bases="all+gm"), "resident_bases"),
    (dict(wide_fused=True, fused_bases="gm", resident_bases="all"), "fused_bases"),
    (dict(wide_fused=True, fused_bases="all+gm", resident_bases="all", dtype="f64"), "f64"),
])
def test_keyword_validation_is_unchanged(kw, match, monkeypatch):
    from revrand_amd import _hip

    def no_device(*a, **k):
        raise AssertionError("a device call before the keywords were checked")
    monkeypatch.setattr(_hip, "get_device", no_device)
    with pytest.raises(ValueError, match=match):
        _glm(**kw).fit(np.zeros((20, 2)), np.zeros(20))
    g = _glm(wide_fused=True, fused_bases="all+gm", resident_bases="all")
    assert g.get_params()["wide_fused"] is True and g.get_params()["fused_bases"] == "all+gm" and g._wide_fused_force is False
