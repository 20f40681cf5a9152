"""Host cost of progressive uploads: the split decoder's entropy decode against PIL's full decode (CPU only).

    python profiles/jpeg_progressive/measure_host.py [--out DIR]

Writes the 100 curated workload images as progressive and as baseline JPEG (q90, 4:2:0: data/synthetic.encode_jpeg's
settings, plus progressive=True), builds csrc/tests/jpeg_entropy_bench.cpp and compact_bench.cpp (next to this file)
with g++ -O2, and prints per file: jpeg_decode_coefs and jpeg_decode_compact on both sets, and
PIL.Image.open(...).convert("RGB") on both sets (fastest of 10 passes, one thread)."""
from __future__ import annotations

import argparse
import io
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def main() -> None:
    from PIL import Image

    from inference_arena_amd.data.curator import workload_images

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for the files and the two programs (default: temporary)")
    out = Path(ap.parse_args().out or tempfile.mkdtemp(prefix="jpeg_progressive_"))
    sets = {"progressive": [], "baseline": []}
    for name, kw in (("progressive", {"progressive": True}), ("baseline", {})):
        (out / name).mkdir(parents=True, exist_ok=True)
        for i, img in enumerate(workload_images()):
            p = out / name / f"{i:03d}.jpg"
            Image.fromarray(img).save(p, format="JPEG", quality=90, **kw)
            sets[name].append(p)
    src = ROOT / "csrc"
    exes = {}
    for exe, main_src in (("entropy", src / "tests" / "jpeg_entropy_bench.cpp"),
                          ("compact", Path(__file__).with_name("compact_bench.cpp"))):
        exes[exe] = out / f"{exe}_bench"
        subprocess.run(["g++", "-O2", "-std=c++17", f"-I{src}", str(main_src), str(src / "runtime" / "jpeg_decode.cpp"),
                        "-o", str(exes[exe])], check=True)
    env = dict(os.environ, ARENA_JPEG_PROGRESSIVE="1")
    for name, files in sets.items():
        size = sum(p.stat().st_size for p in files) / len(files)
        print(f"{name}: {size:.0f} bytes per file")
        for exe, path in exes.items():
            r = subprocess.run([str(path), *map(str, files)], env=env, capture_output=True, text=True, check=True)
            print(f"  {exe:8s} {r.stdout.splitlines()[0]}")
        blobs = [p.read_bytes() for p in files]
        best = 1e30
        for _ in range(10):
            t0 = time.perf_counter()
            for b in blobs:
                with Image.open(io.BytesIO(b)) as im:
                    im.convert("RGB")
            best = min(best, time.perf_counter() - t0)
        print(f"  PIL      {best / len(blobs) * 1e6:.1f} us per image (open + convert('RGB'), best of 10 passes)")


if __name__ == "__main__":
    main()
