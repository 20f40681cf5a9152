"""The fp32 conv family table (csrc/kernels/f32_impl.h) against the numbers that data/tuning/conv_tuning.json holds.

* csrc/tests/f32_impl_check.cpp, built host-only: the valid set, the autotune order and the family lookups equal the
  literals of the on-disk format;
* every shipped table entry of the 14 default programs holds only impls that the executor's add_bucket accepts.
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

from shipped_convs import default_programs as _default_programs  # the 14 default programs, shared

ROOT = Path(__file__).resolve().parents[1]

# ConvParams.impl of an fp32 conv: 119 numbers (the literals of f32_impl_check.cpp)
F32_VALID = {0, 1, 2} | set(range(10, 26)) | set(range(40, 52)) | set(range(100, 167)) | set(range(171, 180)) | \
    {181, 182} | set(range(191, 201))
BF16_VALID = {0, 1, 2, 3}


def test_f32_impl_check_program():
    """The header compiles as plain C++17 without HIP and the check passes."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
                if c and (Path(c).exists() or shutil.which(c))), None)
    if cxx is None:
        pytest.skip("no C++ compiler available")
    src, hdr = ROOT / "csrc" / "tests" / "f32_impl_check.cpp", ROOT / "csrc" / "kernels" / "f32_impl.h"
    exe = ROOT / "build" / "f32_impl_check"
    exe.parent.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or exe.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + str(ROOT / "csrc"), str(src), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "f32_impl_check: ok" in r.stdout, (r.stdout + r.stderr)[-4000:]


def test_shipped_entries_of_the_default_programs_hold_valid_impls():
    from inference_arena_amd.engine import tuning

    assert len(F32_VALID) == 119
    table = tuning.load_table(tuning.DEFAULT_FILE)
    found, bad, programs = 0, [], 0
    for name, dtype, prog in _default_programs():
        programs += 1
        fp = tuning.fingerprint(prog.ops)
        valid = F32_VALID if dtype == "fp32" else BF16_VALID
        for key, entry in table.items():
            if key.split(":")[0] != fp:
                continue
            assert len(entry) == len(prog.ops), (name, dtype, key)
            found += 1
            bad += [(name, dtype, key, i, v) for i, v in enumerate(entry) if v not in valid]
    print(f"{programs} programs, {found} of {len(table)} table entries")
    assert programs == 14
    assert found >= 70, found
    assert not bad, bad[:20]
