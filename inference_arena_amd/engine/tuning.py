"""Persisted conv-kernel selection (deterministic programs across boxes).

The executor can time every conv op of a bucket with each kernel family (bf16:
direct / LDS / pipelined implicit GEMM; fp32: default policy, LDS tile
variants, 3x3 halo tiles)
(csrc/runtime/executor.cpp ``autotune``) and capture the fastest; timing noise
made the choice differ from box to box (impl2:30/impl3:21 on one
box, 27/24 on another), so the same commit ran different programs.  Here the
choices are a table keyed by (program fingerprint, bucket): ``ARENA_TUNING``

* ``table`` (default): use the table entry when present; otherwise tune once,
  store the choices (best effort) and use them;
* ``retune``: tune and overwrite the entry;
* ``off``: no timing, kernel defaults everywhere.

The table lives in ``data/tuning/conv_tuning.json`` (``ARENA_TUNING_FILE``);
tools/tune_programs.py regenerates it on a GPU box.
"""
from __future__ import annotations

import hashlib
import json
import os
import threading
from pathlib import Path

import numpy as np

DEFAULT_FILE = Path(__file__).resolve().parents[2] / "data" / "tuning" / "conv_tuning.json"
_lock = threading.Lock()


def mode() -> str:
    m = os.environ.get("ARENA_TUNING", "table").lower()
    return m if m in ("table", "retune", "off") else "table"


def table_path() -> Path:
    return Path(os.environ.get("ARENA_TUNING_FILE", str(DEFAULT_FILE)))


def fingerprint(ops: np.ndarray) -> str:
    """Program identity: the op records (kinds, shapes, buffer ids, weight offsets), not the weight values."""
    a = np.array(ops, dtype=np.int64)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def load_table(path: Path | None = None) -> dict:
    p = path or table_path()
    try:
        return json.loads(p.read_text())
    except (OSError, ValueError):
        return {}


def lookup(ops: np.ndarray, B: int, path: Path | None = None) -> list[int] | None:
    e = load_table(path).get(f"{fingerprint(ops)}:{B}")
    if e is None or len(e) != len(ops):
        return None
    return [int(v) for v in e]


def store(ops: np.ndarray, B: int, choices: list[int], path: Path | None = None) -> bool:
    """Add one entry.  Several replicas / services that miss the table at start-up store concurrently: the
    load-modify-write runs under an fcntl lock on ``<table>.lock`` (across processes; ``_lock`` within one)
    and the new table goes to a per-process temporary file that is renamed over the table atomically, so a
    reader never sees a torn file and no writer loses another's entry."""
    import fcntl
    import os
    import tempfile

    p = path or table_path()
    with _lock:
        try:
            p.parent.mkdir(parents=True, exist_ok=True)
            with open(p.with_suffix(".lock"), "a+") as lk:
                fcntl.flock(lk.fileno(), fcntl.LOCK_EX)
                try:
                    t = load_table(p)
                    t[f"{fingerprint(ops)}:{B}"] = [int(v) for v in choices]
                    fd, tmp = tempfile.mkstemp(prefix=p.name + ".", suffix=".tmp", dir=str(p.parent))
                    try:
                        with os.fdopen(fd, "w") as f:
                            f.write(json.dumps(t, indent=0, sort_keys=True) + "\n")
                        os.replace(tmp, p)
                    except BaseException:
                        try:
                            os.unlink(tmp)
                        except OSError:
                            pass
                        raise
                finally:
                    fcntl.flock(lk.fileno(), fcntl.LOCK_UN)
            return True
        except OSError:
            return False


def needs_tuning(ops: np.ndarray) -> bool:
    """Conv ops (bf16 and fp32) have kernel families to choose from."""
    from .planner import OP_CONV

    return bool(np.any(ops[:, 0] == OP_CONV))
