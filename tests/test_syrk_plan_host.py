"""The Gram launchers' host-side planner (revrand_amd/csrc/rr_syrk_plan.h) without a GPU.

`test_planner_reproduces_the_recorded_plans`: tests/golden/syrk_plans.json holds what the three launchers launched BEFORE
the planner existed -- a build of that commit that printed, per launcher call, its inputs, the device's CU count, use_map,
od, rg and every kernel with its grid and rows per K-split -- over the shapes of tests/test_gpu_gram_exact.py (every route,
the A/B variants, deterministic mode, the forced K-splits), config 1's and the SARCOS shape, the f64 pairs, the posterior's
square operands, the split engines and the benchmark's 2 000 000 x 4096 chunk, on zero-filled inputs.  rr_syrk_plan, the
C-ABI view of the plan functions the launchers now execute, must return exactly those kernels, grids and rows per split
at the recorded CU count: the first direct test of the split-count searches, which an exact Gram cannot see.  Cases under
switches read once per process run in a child process per switch setting.

`test_plan_sweep_under_sanitizers`: tests/syrk_plan_sweep.cpp, the header alone under the host compiler with
-fsanitize=address,undefined, holds every plan of a shape sweep to the invariants the kernels rely on.
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT

# rr_syrk_plan's kernel codes (include/revrand_hip.h) by the names the recording printed
KERNEL_CODES = {"rr_syrk_f32_small_kernel": 1, "rr_syrk_f32_kernel": 2, "rr_syrk_f32_w8_kernel": 3, "rr_syrk_f32_flat_kernel": 4,
                "rr_syrk_f32_flatstag_kernel": 5, "rr_syrk_f32_buf_kernel": 6, "rr_syrk_f32_ragged_kernel": 7,
                "rr_syrk_f32_diag_kernel": 8, "rr_syrk_f32_diag16_kernel<32>": 9, "rr_syrk_f32_diag16_kernel<64>": 10,
                "rr_syrk_f32_merged_kernel": 11, "rr_syrk_f64_kernel": 12, "rr_syrk_f64_diag_kernel": 13,
                "rr_syrk_b16w4_kernel": 14}
NOT_PLANNED = ("rr_syrk_det_reduce_kernel", "rr_split_bf16_kernel")   # their grids follow from the shape alone
LAUNCHERS = {"f32": 0, "f64": 1, "b16": 2}
# the switches the launchers read once per process, and those they read on every call
ONCE = ("RR_SYRK_SMALL", "RR_SYRK_SPLIT_SEARCH", "RR_SYRK_STAGGER", "RR_SYRK_W8", "RR_SYRK_MERGE_DIAG", "RR_SYRK_NO_DIAG16",
        "RR_SYRK_DIAG_KB", "RR_SYRK64_FINE_SPLIT", "RR_SYRK64_TRI")
PER_CALL = ("RR_GRAM_ROWS_PER_SPLIT", "RR_GRAM_NO_TILE_MAP", "RR_SYRK_NO_DIAG_KERNEL", "RR_SYRK_NO_RAGGED_KERNEL", "RR_GRAM_ABLATE")


def _recorded():
    with open(os.path.join(GOLDEN, "syrk_plans.json")) as f:
        return json.load(f)


def _kernel_code(name):
    name = name.strip("()")
    if name.startswith("rr_syrk_b16w4_kernel<"):
        name = "rr_syrk_b16w4_kernel"
    return KERNEL_CODES[name]


def expected(entry):
    """What rr_syrk_plan must return for a recorded launcher call: (header fields, [(kernel, grid, rows per split)])."""
    kernels = [(_kernel_code(n), g, r) for n, g, r in entry["kernels"] if not n.strip("()").startswith(NOT_PLANNED)]
    reduce = any(n.startswith("rr_syrk_det_reduce_kernel") for n, _, _ in entry["kernels"])
    head = {"use_map": entry["use_map"], "od": entry["od"], "rg": entry["rg"], "nb": entry["nb"], "ntiles": entry["ntiles"],
            "reduce": reduce}
    return head, kernels


def planned(lib, entry):
    """rr_syrk_plan for the inputs of a recorded call, in the same form (the merged launch as the one launch it is)."""
    import ctypes
    out = (ctypes.c_int64 * 22)()
    n = lib.rr_syrk_plan(LAUNCHERS[entry["launcher"]], entry["rows"], entry["ldp"], entry["F"], entry["flag"], entry["num_cu"],
                         entry["det"], out, 22)
    assert n == 22 and out[0] == 0, (n, out[0])
    head = {"use_map": out[7], "od": out[5], "rg": out[6], "nb": out[3], "ntiles": out[4], "reduce": out[8] > 0}
    parts = [tuple(out[i:i + 3]) for i in (10, 14, 18) if out[i]]
    if out[1] == 2:   # merged: both parts in one launch, the off-diagonal tiles' rows per split first
        assert [p[0] for p in parts] == [11, 11]
        assert (entry["merged_n_off"], entry["merged_rps_d"]) == (parts[0][1], parts[1][2]), (entry, parts)
        parts = [(11, parts[0][1] + parts[1][1], parts[0][2])]
    if out[8]:        # one slab per K-split, shared by every kernel of the route
        assert {out[i + 3] for i in (10, 14, 18) if out[i]} == {out[8]}
    return head, parts


def check_group(static_env):
    """In a process started under static_env: every recorded call of that group against rr_syrk_plan; the mismatches."""
    from revrand_amd import _hip
    lib = _hip.load_library()
    bad, n = [], 0
    for entry in _recorded():
        if {k: v for k, v in entry["env"].items() if k in ONCE} != static_env:
            continue
        for k in PER_CALL:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in entry["env"].items() if k in PER_CALL})
        n += 1
        want, got = expected(entry), planned(lib, entry)
        if want != got:
            bad.append("%s %s: recorded %s, planned %s" % (entry["case"], entry["env"], want, got))
    return n, bad


def _groups():
    seen = []
    for entry in _recorded():
        env = {k: v for k, v in entry["env"].items() if k in ONCE}
        assert set(entry["env"]) <= set(ONCE + PER_CALL), entry["env"]
        if env not in seen:
            seen.append(env)
    return seen


def test_recording_covers_the_case_list():
    """Every launcher, every kernel but the opt-in 8-wave one, the deterministic reduction, both tile-map settings, forced
    K-splits, and the shapes the split choices were tuned on are in the recording, at one CU count."""
    rec = _recorded()
    assert len({e["num_cu"] for e in rec}) == 1 and len(rec) >= 200
    assert {e["launcher"] for e in rec} == set(LAUNCHERS)
    seen = {_kernel_code(n) for e in rec for n, _, _ in e["kernels"] if not n.strip("()").startswith(NOT_PLANNED)}
    assert seen == set(KERNEL_CODES.values()) - {3}, sorted(seen)
    assert any(e["det"] for e in rec if e["launcher"] == "f32") and any(e["det"] for e in rec if e["launcher"] == "f64")
    assert {e["use_map"] for e in rec} == {0, 1} and any("RR_GRAM_ROWS_PER_SPLIT" in e["env"] for e in rec)
    shapes = {(e["launcher"], e["rows"], e["F"], e["flag"]) for e in rec}
    assert {("f32", 10016, 512, 0), ("f32", 10016, 500, 1), ("f32", 44512, 1024, 0), ("f32", 2000000, 4096, 0),
            ("f64", 512, 512, 1), ("f64", 1024, 1024, 1), ("f64", 2048, 2048, 1), ("b16", 40000, 4096, 1)} <= shapes
    assert len(_groups()) == 9 and {} in _groups()


@pytest.mark.parametrize("static_env", _groups(), ids=lambda v: ",".join("%s=%s" % kv for kv in sorted(v.items())) or "default")
def test_planner_reproduces_the_recorded_plans(static_env):
    code = ("import json, sys; sys.path[:0] = [%r, %r]\nimport test_syrk_plan_host as T\n"
            "print('PLANRESULT', json.dumps(T.check_group(%r)))\n" % (ROOT, os.path.join(ROOT, "tests"), static_env))
    env = {k: v for k, v in os.environ.items() if k not in ONCE and k not in PER_CALL}
    env.update(static_env)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("PLANRESULT ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    n, bad = json.loads(lines[-1][len("PLANRESULT "):])
    assert n >= 10 and bad == [], "%d of %d plans differ:\n%s" % (len(bad), n, "\n".join(bad[:20]))


def test_plan_sweep_under_sanitizers(tmp_path):
    """tests/syrk_plan_sweep.cpp with the host compiler under AddressSanitizer and UBSan, run directly: exit status 0,
    its closing line, and no sanitizer report."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "syrk_plan_sweep")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "revrand_amd", "csrc"), os.path.join(ROOT, "tests", "syrk_plan_sweep.cpp"), "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ONCE and k not in PER_CALL}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "plans hold" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-3000:])
