"""The one-wave-per-SIMD body of rr_syrk_f32_kernel (rr_syrk_f32_w4_body, rr_rff.hip) at the edges of its LDS ring.

The kernel walks a K-split in stages of 16 rows through a ring of four LDS stages, unrolled by the ring: a split of S stages
(S even, rows per split being multiples of 32) runs S // 4 whole turns and, for S = 2 (mod 4), half a turn; S = 2 is fewer
stages than the ring holds, and past the end of a split the DMA fetches the last stage again.  The cases:

* ring edges: 32 .. 224 rows in ONE split (2, 4, 6, 8, 10, 14 stages) on one off-diagonal tile (F = 500) and on the lone
  diagonal tile of a one-block Gram (F = 200, where the wave below the diagonal only moves data), with and without y;
* K-splits of 32, 64, 96, 1024 rows and the launcher's own over 4000 rows (the last split shorter than the rest);
* the 120-tile map on and off, and the ragged kernel beside it.

All of these are exact on integer data (tests/test_gpu_gram_exact.py: Phi in [-3, 3], y in [-2, 2], `==` against NumPy).
On uniform random floats in deterministic mode the kernel must give the bits of the 8-wave body it replaced
(RR_SYRK_W8=1): the two share the per-split summation order and nothing else.  Under the bounds-checking build each
Gram launches the kernel the switch names exactly once and no guard band or device assertion reports.

RR_SYRK_SMALL=0 (F <= 1024 at these row counts would take the 128 x 128 kernel) and RR_SYRK_W8 are read once per process,
so those cases run in child processes, one after another through `guarded_child` of tests/test_gpu_gram_exact.py: after a
child that failed, reported a violation or ran into its time limit none is started.
"""
import os

import numpy as np
import pytest

import test_gpu_gram_exact as E
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
ONE_SPLIT = {"RR_GRAM_ROWS_PER_SPLIT": "4096"}           # every row of a ring-edge case in one K-split: S = rows / 16
RING_ROWS = [32, 64, 96, 128, 160, 224]                  # 2, 4, 6, 8, 10, 14 stages
RING_F = [500, 200]                                      # one off-diagonal tile (+ diag16) / nb_all = 1: the diagonal tile
KSPLIT_ROWS = 4000
KSPLIT_F = [500, 1100, 1280]                             # 1 tile; 6 tiles + ragged; 10 tiles, no rider
KSPLIT_RPS = ["32", "64", "96", "1024", None]
MAP_CASES = [(1000, 4096, {}), (1000, 4096, {"RR_GRAM_NO_TILE_MAP": "1"}), (1000, 4100, {})]
# (rows, F, with y, per-call switches) of groups 1-3
RING_CASES = [(rows, F, y, ONE_SPLIT) for F in RING_F for rows in RING_ROWS for y in (False, True)]
KSPLIT_CASES = [(KSPLIT_ROWS, F, True, {"RR_GRAM_ROWS_PER_SPLIT": rps} if rps else {}) for F in KSPLIT_F for rps in KSPLIT_RPS]
ALL_CASES = RING_CASES + KSPLIT_CASES + [(rows, F, False, env) for rows, F, env in MAP_CASES]
# one case per route for the comparison with the 8-wave body
SAME_BITS_CASES = [(224, 500, True, ONE_SPLIT), (96, 500, False, ONE_SPLIT), (160, 200, True, ONE_SPLIT),
                   (KSPLIT_ROWS, 1100, True, {"RR_GRAM_ROWS_PER_SPLIT": "96"}), (KSPLIT_ROWS, 1280, True, {}),
                   (1000, 4096, False, {}), (1000, 4100, False, {})]
NO_SMALL = {"RR_SYRK_SMALL": "0"}
CHILD = "sys.path.insert(0, %r)\nimport test_gpu_gram_w4 as W\n" % os.path.join(ROOT, "tests")


def _label(case):
    rows, F, with_y, env = case
    return "gram(%d, %d%s)%s" % (rows, F, ", y" if with_y else "", " %s" % (sorted(env.items()),) if env else "")


def _main_route(case, environ):
    """The case must reach the main kernel with at least one tile (else it would say nothing about this kernel)."""
    rows, F, with_y, env = case
    r = E.f32_route(rows, F, E.takes_rider(F, with_y), E._device().compute_units, dict(environ, **env))
    assert r["kind"] == "main" and r["ntiles"] > 0, (_label(case), r)
    return r


def exact_child(cases):
    """Mismatches of `cases` against the exact integer references under this process' switches ([] when all are exact)."""
    bad = []
    for case in cases:
        rows, F, with_y, env = case
        _main_route(case, os.environ)
        Phi, y, G, b, yty = E._case(rows, F)
        Gd, bd, td = E.run_gram(Phi, y if with_y else None, env=env)
        bad += [m for m in (E._mismatch(Gd, G, _label(case) + ": G"),) if m]
        if with_y:
            bad += [m for m in (E._mismatch(bd, b, _label(case) + ": b"), "" if td == yty else _label(case) + ": yty") if m]
    return bad


def _float_case(rows, F):
    rs = np.random.RandomState(rows * 104729 + F)
    return rs.uniform(-1.0, 1.0, size=(rows, F)).astype(np.float32), rs.uniform(-1.0, 1.0, size=rows).astype(np.float32).astype(np.float64)


def bits_child(out_dir):
    """Deterministic-mode Grams of SAME_BITS_CASES on uniform random floats, saved as <out_dir>/<index>.npz."""
    for n, case in enumerate(SAME_BITS_CASES):
        rows, F, with_y, env = case
        _main_route(case, os.environ)
        Phi, y = _float_case(rows, F)
        G, b, _ = E.run_gram(Phi, y if with_y else None, env=env, det=True)
        np.savez(os.path.join(out_dir, "%d.npz" % n), G=G, b=b)
    return len(SAME_BITS_CASES)


def census_child(cases):
    """[(label, launches of rr_syrk_f32_kernel, of rr_syrk_f32_w8_kernel, mismatch of G or '')] of one Gram per case under a
    library that counts launches (the bounds-checking build); dev.sync() inside verifies the guard bands."""
    lib = E._device().lib
    assert lib.rr_debug_kernel_launches(None) == 0
    out = []
    for case in cases:
        rows, F, with_y, env = case
        _main_route(case, os.environ)
        Phi, y, G = E._case(rows, F)[:3]
        E._device().sync()
        lib.rr_debug_kernel_launches(None)
        Gd = E.run_gram(Phi, y if with_y else None, env=env)[0]
        out.append((_label(case), int(lib.rr_debug_kernel_launches(b"rr_syrk_f32_kernel")),
                    int(lib.rr_debug_kernel_launches(b"rr_syrk_f32_w8_kernel")), E._mismatch(Gd, G, _label(case))))
    return out


# ---- 1, 2: the cases that need RR_SYRK_SMALL=0 run in one child each ------------------------------------------------------
def test_ring_edges_are_exact():
    """2 to 14 stages in one K-split -- fewer than the ring holds, S = 2 (mod 4), wrap-around -- on an off-diagonal tile and on
    the diagonal tile of a one-block Gram, with and without the rider."""
    bad = E.guarded_child("the ring edges", CHILD + "print('W4RESULT', json.dumps(W.exact_child(W.RING_CASES)))\n",
                          dict(NO_SMALL, RR_SYRK_W8="0"), "W4RESULT", timeout=300)
    assert bad == []


def test_k_splits_of_one_tile_are_exact():
    """F = 500 over 4000 rows at every split geometry: one off-diagonal tile, which the 128 x 128 kernel would take."""
    code = CHILD + "print('W4RESULT', json.dumps(W.exact_child([c for c in W.KSPLIT_CASES if c[1] == 500])))\n"
    assert E.guarded_child("the K-splits at F = 500", code, dict(NO_SMALL, RR_SYRK_W8="0"), "W4RESULT", timeout=300) == []


@pytest.mark.parametrize("rps", KSPLIT_RPS, ids=lambda r: "rps=%s" % r)
@pytest.mark.parametrize("F", [F for F in KSPLIT_F if F > 1024])
def test_k_splits_are_exact(F, rps):
    """Splits of 2, 4 and 6 stages, 64 stages with a last split of 58, and the launcher's own; the last split shorter."""
    case = (KSPLIT_ROWS, F, True, {"RR_GRAM_ROWS_PER_SPLIT": rps} if rps else {})
    _main_route(case, os.environ)
    E._check_case(KSPLIT_ROWS, F, True, env=case[3])


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,F,env", MAP_CASES, ids=["%dx%d%s" % (r, F, "-nomap" if e else "") for r, F, e in MAP_CASES])
def test_map_and_ragged_neighbours_are_exact(rows, F, env):
    """120 tiles through the XCD tile map and in plain order, and the same 120 beside the ragged kernel's 16."""
    r = _main_route((rows, F, False, env), os.environ)
    assert r["ntiles"] == 120 and r["use_map"] == (not env) and r["rg"] == (1 if F == 4100 else 0), r
    E._check_case(rows, F, False, env=env, last_block=(F - 1) // 256 * 256)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def test_same_bits_as_the_eight_wave_body(tmp_path):
    """Deterministic mode on uniform random floats: G and b of one case per route are the bits RR_SYRK_W8=1 gives."""
    dirs = {}
    for arm in ("1", "0"):
        dirs[arm] = tmp_path / ("w8_" + arm)
        dirs[arm].mkdir()
        n = E.guarded_child("the same-bits Grams under RR_SYRK_W8=%s" % arm,
                            CHILD + "print('W4RESULT', json.dumps(W.bits_child(%r)))\n" % str(dirs[arm]),
                            dict(NO_SMALL, RR_SYRK_W8=arm), "W4RESULT", timeout=300)
        assert n == len(SAME_BITS_CASES)
    for n, case in enumerate(SAME_BITS_CASES):
        with np.load(str(dirs["1"] / ("%d.npz" % n))) as old, np.load(str(dirs["0"] / ("%d.npz" % n))) as new:
            assert np.abs(old["G"]).max() > 0 and np.isfinite(new["G"]).all(), _label(case)
            assert np.array_equal(old["G"], new["G"]), (_label(case), "G", int((old["G"] != new["G"]).sum()))
            assert np.array_equal(old["b"], new["b"]), (_label(case), "b", int((old["b"] != new["b"]).sum()))
            if case[2]:
                assert np.abs(new["b"]).max() > 0, _label(case)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["default", "RR_SYRK_W8=1"])
def test_bounds_build_counts_one_launch_and_reports_nothing(arm):
    """Every case above under the bounds-checking build: the default launches rr_syrk_f32_kernel once per Gram and
    rr_syrk_f32_w8_kernel never, RR_SYRK_W8=1 the other way round; no guard band, no RR_DEV_ASSERT reports; exact."""
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    w8 = arm != "default"
    rows = E.guarded_child("the launch counts under %s" % arm, CHILD + "print('W4RESULT', json.dumps(W.census_child(W.ALL_CASES)))\n",
                           dict(NO_SMALL, RR_SYRK_W8="1" if w8 else "0", REVRAND_HIP_LIB=DEBUG_LIB), "W4RESULT", timeout=600,
                           forbidden=("RR_BOUNDS",))
    assert [r[0] for r in rows] == [_label(c) for c in ALL_CASES]
    bad = [r for r in rows if (r[1], r[2]) != ((0, 1) if w8 else (1, 0)) or r[3]]
    assert not bad, bad
