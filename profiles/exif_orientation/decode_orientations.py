"""32 uploads of 640x480 4:2:0 per orientation through jpeg_decode_device (kernel timing under rocprofv3)."""
import io, sys
sys.path[:0] = [".", "tests"]
import numpy as np
import exif_cases as X
from inference_arena_amd.ops import native
C = native()
frames = [X.scene(480, 640, seed=i) for i in range(32)]
for rep in range(3):
    for o in range(1, 9):
        ups = [X.encode(f, "420") if o == 1 else X.tagged(f, "420", o, "le") for f in frames]
        out = C.jpeg_decode_device(ups, 0)
        assert out[0].shape == ((640, 480, 3) if o >= 5 else (480, 640, 3))
print("done")
