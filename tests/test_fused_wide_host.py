"""The host side of the wide small-minibatch loop (rr_glm_sviw, rr_svi_wide.hip; GeneralizedLinearModel(wide_fused=True)):
the keyword, the range check and the planner that cuts a step into work items.  None of it needs a device."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _glm(**kw):
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.glm import GeneralizedLinearModel
    return GeneralizedLinearModel(lk.Gaussian(), bs.RandomRBF(nbases=6, Xdim=2, random_state=0), maxiter=3, nstarts=0, **kw)


def test_keyword_is_a_parameter_of_the_estimator():
    from sklearn.base import clone
    g = _glm()
    assert g.get_params()["wide_fused"] is False
    g = _glm(wide_fused=True)
    assert g.get_params()["wide_fused"] is True
    assert clone(g).wide_fused is True
    assert pickle.loads(pickle.dumps(g)).wide_fused is True
    assert g._wide_fused_force is False


@pytest.mark.parametrize("bad", ["yes", 1, 0, None, "True"])
def test_bad_value_is_refused_before_any_device_call(bad, monkeypatch):
    from revrand_amd import _hip

    def no_device(*a, **k):
        raise AssertionError("a device call before the keyword was checked")
    monkeypatch.setattr(_hip, "get_device", no_device)
    X, y = np.zeros((20, 2)), np.zeros(20)
    with pytest.raises(ValueError, match="wide_fused"):
        _glm(wide_fused=bad).fit(X, y)


def test_float64_step_refuses_the_wide_loop(monkeypatch):
    from revrand_amd import _hip

    def no_device(*a, **k):
        raise AssertionError("a device call before the keyword was checked")
    monkeypatch.setattr(_hip, "get_device", no_device)
    with pytest.raises(ValueError, match="wide_fused"):
        _glm(wide_fused=True, dtype="f64").fit(np.zeros((20, 2)), np.zeros(20))


def test_header_exports_and_ctypes_entries_agree():
    from revrand_amd import _hip
    src = open(os.path.join(ROOT, "include", "revrand_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rr_glm_sviw_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["rr_glm_sviw_" + n for n in ("create", "destroy", "plan", "read", "run", "set_start", "starts", "supported")]
    lib = _hip.load_library()
    for name in declared:
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    for m in ("set_start", "run", "starts", "read", "close"):
        assert callable(getattr(_hip.WideSvi, m))
    assert _hip.WideSvi.run is not _hip.FusedSvi.run and _hip.WideSvi.starts is not _hip.FusedSvi.starts


def test_supported_range():
    from revrand_amd import _hip
    for F in (512, 1024, 2048, 4096, 8192, 16384, 32768):   # the report's nbases 256 ... 8192 and the documented edge
        assert _hip.sviw_supported(F, 10, 50, 10, 1, 21, 21), F
    assert _hip.sviw_supported(36, 3, 6, 64, 3, 12, 5)
    assert _hip.sviw_supported(1356, 3, 6, 10, 3, 15, 6)
    assert _hip.sviw_supported(2048, 32, 3, 64, 1, 128, 128)      # each documented edge
    assert _hip.sviw_supported(2048, 8, 128, 16, 16, 128, 0)
    assert not _hip.sviw_supported(512, 33, 50, 10, 1, 21, 21)    # K = 33
    assert not _hip.sviw_supported(512, 10, 50, 10, 17, 21, 21)   # 17 children
    assert not _hip.sviw_supported(0, 10, 50, 10, 1, 21, 21)      # F = 0
    assert not _hip.sviw_supported(32770, 10, 50, 10, 1, 21, 21)
    assert not _hip.sviw_supported(512, 10, 129, 10, 1, 21, 21)
    assert not _hip.sviw_supported(512, 10, 50, 65, 1, 21, 21)
    # the upper edge in minibatch x F follows the measured per-step times (docs/KERNELS.md 3.48): inside, the chain won by 2.2 x
    # or more; the shapes it won by 1.2 x or lost are declined
    assert _hip.sviw_supported(2048, 10, 50, 32, 1, 21, 21)
    assert not _hip.sviw_supported(2048, 10, 50, 64, 1, 21, 21)
    assert not _hip.sviw_supported(16384, 10, 50, 32, 1, 21, 21)
    assert not _hip.sviw_supported(16384, 10, 50, 64, 1, 21, 21)


def _check_plan(children, K, L, M, width=None):
    """the items tile every child's frequencies / columns exactly once, in order; none straddles a child; LDS within budget"""
    from revrand_amd import _hip
    items, info = _hip.sviw_plan(children, K, L, M)
    assert info["items"] == len(items) and info["lds_bytes"] <= info["lds_budget"] <= 160 * 1024
    if width is not None:
        assert info["width"] == width
    pos = 0
    for c, ch in enumerate(children):
        total = ch[1] if ch[0] == "rff" else ch[1] + (1 if ch[2] else 0)
        mine = []
        while pos < len(items) and items[pos][0] == c:
            mine.append(items[pos])
            pos += 1
        assert mine, "child %d has no item" % c
        if ch[0] == "linear":
            assert mine == [(c, 0, total)]      # one item, whatever its width
            continue
        nxt = 0
        for (_, j0, cnt) in mine:
            assert j0 == nxt and 1 <= cnt <= info["width"]
            nxt += cnt
        assert nxt == total
        assert all(cnt == info["width"] for (_, _, cnt) in mine[:-1])
    assert pos == len(items)
    return items, info


_PLAN_CODE = """
import sys, json
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_fused_wide_host as t
from revrand_amd import _hip
_, info = _hip.sviw_plan([("rff", 1000, 5)], 10, 50, 10)
item = info["width"]
out = {"item": item}
for n in (1, item - 1, item, item + 1, int(2.5 * item)):
    for lin in (None, True, False):
        kids = [("rff", n, 5)] + ([] if lin is None else [("linear", 5, lin)]) + [("rff", 3, 3)]
        items, inf = t._check_plan(kids, 10, 50, 10, width=item)
        out["%%d/%%s" %% (n, lin)] = len(items)
print("PLAN " + json.dumps(out))
"""


@pytest.mark.parametrize("env", ["8", "16", None])
def test_plan_tiles_every_child(env):
    """RR_SVIW_ITEM is read by the library: each value in a process of its own."""
    e = dict(os.environ)
    e.pop("RR_SVIW_ITEM", None)
    if env is not None:
        e["RR_SVIW_ITEM"] = env
    r = subprocess.run([sys.executable, "-c", _PLAN_CODE % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       timeout=300, env=e, cwd=os.path.join(ROOT, "tests"))
    assert r.returncode == 0 and "PLAN " in r.stdout, r.stderr[-3000:]
    import json
    out = json.loads(r.stdout.split("PLAN ", 1)[1])
    item = out["item"]
    assert item == (int(env) if env is not None else 64)
    # n = item + 1: two items for that child; 2.5 item: three; plus the linear child's one and the third child's
    assert out["%d/None" % (item + 1)] == 2 + 1 and out["%d/True" % int(2.5 * item)] == 3 + 1 + 1
    assert out["1/False"] == 1 + 1 + 1


def test_plan_width_follows_the_lds_budget():
    """the widest shape the range admits: the width shrinks until an item fits, and never below one frequency"""
    _, info = _check_plan([("rff", 300, 128), ("linear", 128, True)], 32, 128, 64)
    assert 1 <= info["width"] < 64
    _, info = _check_plan([("rff", 8192, 21)], 10, 50, 10)
    assert info["width"] == 64 and info["items"] == 128
    from revrand_amd import _hip
    with pytest.raises(ValueError):
        _hip.sviw_plan([("centres", 10, 2)], 4, 10, 10)
