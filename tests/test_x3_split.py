"""The triple-bf16 split (csrc/kernels/x3.h): one rule for the kernels, the host and the weight packer.

* csrc/tests/x3_split_check.cpp, built host-only with clang: the element-wise and the two-at-a-time form of the split
  give identical plane bits on fixed edge values and on 1.04e7 random bit patterns, and h + m + l == v exactly
  wherever the arithmetic guarantees it (the program states and counts what it leaves out);
* engine/planner.py split_bf16x3, which packs the pre-split weights, gives the planes of that program on the same
  edge values.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
SRC, HDR = ROOT / "csrc" / "tests" / "x3_split_check.cpp", ROOT / "csrc" / "kernels" / "x3.h"


def _clang():
    """A clang++ (the header needs __bf16 and ext_vector_type on the host), or None."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.environ.get("CXX"), "clang++", rocm + "/llvm/bin/clang++", rocm + "/lib/llvm/bin/clang++"):
        path = c and (c if Path(c).exists() else shutil.which(c))
        if not path:
            continue
        r = subprocess.run([path, "--version"], capture_output=True, text=True, timeout=60)
        if r.returncode == 0 and "clang" in r.stdout:
            return path
    return None


@pytest.fixture(scope="module")
def check_run():
    """(stdout, planes file) of one run of the check program."""
    cxx = _clang()
    if cxx is None:
        pytest.skip("no clang++ available")
    exe, planes = ROOT / "build" / "x3_split_check", ROOT / "build" / "x3_split_planes.bin"
    exe.parent.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or exe.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        cmd = [cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + str(ROOT / "csrc"), str(SRC), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe), str(planes)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "x3_split_check: ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    return r.stdout, planes


def test_both_forms_give_the_same_planes_and_sum_back_exactly(check_run):
    out, _ = check_run
    print(out.strip())
    n = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out)}
    assert n["values"] >= 10_000_000
    assert n["values"] == n["exact"] + n["left_out_overflow"] + n["left_out_subnormal"]
    assert n["exact"] >= n["normal_l"]
    # nothing is left out of a value whose fp32 quantum is at least 2^-126 (biased exponent 24 .. 254, 231 of the 255
    # exponents of a random non-NaN pattern = 0.906) unless it rounds past bf16's range (under 1e-4 of them)
    assert n["exact"] > 0.9 * n["values"]


def test_planner_split_gives_the_planes_of_the_header(check_run):
    from inference_arena_amd.engine.planner import split_bf16x3

    _, planes = check_run
    rec = np.fromfile(planes, dtype=np.dtype([("v", "<u4"), ("p", "<u2", (3,))]))
    assert len(rec) == 48
    v = torch.from_numpy(rec["v"].copy().view(np.float32))
    assert {0.0, float("inf"), float("-inf")} <= set(v.tolist())
    got = split_bf16x3(v).view(torch.int16).numpy().view(np.uint16)  # [3, N]
    want = rec["p"].T
    nan = lambda b: (b & 0x7FFF) > 0x7F80  # noqa: E731  (±inf and values past bf16's range: m and l are NaN)
    both_nan = nan(got) & nan(want)
    bad = np.argwhere((got != want) & ~both_nan)
    assert bad.size == 0, [(hex(rec["v"][i]), p, hex(got[p, i]), hex(want[p, i])) for p, i in bad[:8]]
    assert not both_nan[0].any() and both_nan.sum() < 2 * 8  # h is never NaN; only the overflowing few have NaN m, l
