"""JPEG files PIL cannot write, for the layout tests (test_jpeg_layouts.py, test_jpeg_layouts_gpu.py): any sampling
factors, any split of the components over scans, RGB-coded components, and progressive twins.

PIL writes 4:4:4, 4:2:2 and 4:2:0 in one scan only (``subsampling`` 3, 4 and "4:1:1" silently give 4:2:0), so this is
a small baseline writer in numpy: float DCT, quantisation with the tables of a PIL file, Huffman coding with the DHT
segments of a PIL file (both read from a file PIL writes at run time: nothing is typed in here).  The pixel oracle of
every file is PIL's decode of it, so the writer only has to produce valid files, not good ones.

``python tests/jpeg_layout_cases.py`` (or ``self_test()``) checks the writer itself: PIL opens every case as RGB, and
the writer's 4:2:0 single-scan control is decoded by the split decoder's host half exactly as PIL decodes it."""
from __future__ import annotations

import functools
import io
import struct

import numpy as np
from PIL import Image

# (h, w): a one-row chroma plane, both parities of the last row, widths on both sides of a 32-wide MCU
SIZES = [(37, 53), (16, 16), (9, 7), (1, 1), (3, 101), (101, 3), (33, 17), (17, 33)]

S444 = [(1, 1), (1, 1), (1, 1)]
S420 = [(2, 2), (1, 1), (1, 1)]
S440 = [(1, 2), (1, 1), (1, 1)]
S411 = [(4, 1), (1, 1), (1, 1)]
# name -> sampling factors of Y, Cb, Cr; the split decoder's layout number and (rh, rv) for each
SAMPLINGS = {
    "440": (S440, 4, (1, 2)),
    "440_h2": ([(2, 2), (2, 1), (2, 1)], 4, (1, 2)),
    "411": (S411, 5, (4, 1)),
    "410": ([(4, 2), (1, 1), (1, 1)], 5, (4, 2)),
    "311": ([(3, 1), (1, 1), (1, 1)], 5, (3, 1)),
    "1x4": ([(1, 4), (1, 1), (1, 1)], 5, (1, 4)),
    "2x4": ([(2, 4), (1, 1), (1, 1)], 5, (2, 4)),
}
SCAN_SCRIPTS = {"y_cb_cr": [[0], [1], [2]], "cr_y_cb": [[2], [0], [1]], "y_cbcr": [[0], [1, 2]]}

_ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
           14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
           53, 60, 61, 54, 47, 55, 62, 63]


def scene(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([x / max(w, 1) * 200, y / max(h, 1) * 180, (x + y) / max(h + w, 1) * 150], -1)
    img += rng.normal(0, 25, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def segments(data: bytes):
    """[(marker, start, end)] of a well-formed file; an SOS segment extends over its entropy-coded data."""
    out, pos = [(0xD8, 0, 2)], 2
    while pos < len(data):
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        if m == 0xD9:
            out.append((m, pos, pos + 2))
            break
        end = pos + 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        if m == 0xDA:
            while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
                end += 1
        out.append((m, pos, end))
        pos = end
    return out


def join(data: bytes, segs) -> bytes:
    return b"".join(data[a:b] for _, a, b in segs)


@functools.lru_cache(maxsize=None)
def _tables(quality=90):
    """From a file PIL writes: the JFIF APP0 segment, the two quantisation tables (zigzag order, as a DQT holds
    them), the DHT segments as they are, and the codes {(class, id): {symbol: (code, length)}} they define."""
    b = io.BytesIO()
    Image.fromarray(scene(16, 16, 1)).save(b, "JPEG", quality=quality, subsampling=0)
    data = b.getvalue()
    app0, qt, dht, codes = b"", {}, b"", {}
    for m, a, e in segments(data):
        seg = data[a + 4:e]
        if m == 0xE0:
            app0 = data[a:e]
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                assert seg[q] >> 4 == 0
                qt[seg[q] & 15] = np.frombuffer(seg[q + 1:q + 65], np.uint8).astype(np.int32)
                q += 65
        elif m == 0xC4:
            dht += data[a:e]
            q = 0
            while q < len(seg):
                key = (seg[q] >> 4, seg[q] & 15)
                counts = seg[q + 1:q + 17]
                vals = seg[q + 17:q + 17 + sum(counts)]
                table, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[vals[k]] = (code, length)
                        code += 1
                        k += 1
                    code <<= 1
                codes[key] = table
                q += 17 + len(vals)
    assert app0 and set(qt) == {0, 1} and set(codes) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    return app0, qt, dht, codes


@functools.lru_cache(maxsize=None)
def _dct_matrix():
    k, n = np.mgrid[0:8, 0:8].astype(np.float64)
    m = np.cos((2 * n + 1) * k * np.pi / 16) / 2
    m[0] /= np.sqrt(2)
    return m


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def _put_dc(bits, table, diff):
    s, extra = _magnitude(diff)
    bits.put(*table[s])
    if s:
        bits.put(extra, s)


def _put_ac(bits, table, zz):
    run = 0
    last = max((k for k in range(1, 64) if zz[k]), default=0)
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*table[0xF0])
            run -= 16
        s, extra = _magnitude(int(zz[k]))
        bits.put(*table[(run << 4) | s])
        bits.put(extra, s)
        run = 0
    if last < 63:
        bits.put(*table[0x00])


def _blocks(plane, qt):
    """Quantised coefficients int32[bh][bw][64] in zigzag order of a plane whose sides are multiples of 8."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.astype(np.float64).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128.0
    m = _dct_matrix()
    c = m @ x @ m.T
    zz = c.reshape(bh, bw, 64)[:, :, _ZIGZAG]
    return np.rint(zz / qt).astype(np.int32)


def write(planes, sampling=S420, scans=None, restart=0, ids=(1, 2, 3), jfif=True, adobe=None, progressive=False,
          between=None, quality=90) -> bytes:
    """A JPEG whose three components are the channels of `planes` (HxWx3 uint8), component c subsampled by box
    averaging to its factors sampling[c] = (h, v), quantised with the tables PIL uses at `quality`.  The other
    arguments are write_coefs's."""
    _, qt, _, _ = _tables(quality)
    H, W = planes.shape[:2]
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    full = np.pad(planes, ((0, mcuy * 8 * vmax - H), (0, mcux * 8 * hmax - W), (0, 0)), mode="edge").astype(np.float64)
    blocks = []
    for c, (h, v) in enumerate(sampling):
        assert hmax % h == 0 and vmax % v == 0
        fh, fv = hmax // h, vmax // v
        p = full[:, :, c].reshape(mcuy * 8 * v, fv, mcux * 8 * h, fh).mean(axis=(1, 3))
        blocks.append(_blocks(np.clip(np.rint(p), 0, 255), qt[0 if c == 0 else 1]))
    return write_coefs((H, W), blocks, qt, sampling, scans=scans, restart=restart, ids=ids, jfif=jfif, adobe=adobe,
                       progressive=progressive, between=between)


def write_coefs(size, blocks, qt, sampling=S444, pq=(0, 0), scans=None, restart=0, ids=(1, 2, 3), jfif=True,
                adobe=None, progressive=False, between=None) -> bytes:
    """A JPEG of size = (H, W) from quantised coefficients: blocks[c] is int[mcuy * v][mcux * h][64] in zigzag order
    for component c with factors sampling[c] = (h, v); qt = {0: luma table, 1: chroma table}, 64 entries each in
    zigzag order, written with 16-bit entries (DQT precision Pq = 1) where pq[t] is 1.  The Huffman tables are PIL's
    (DC differences up to +-2047, AC coefficients up to +-1023): the caller keeps the blocks within them.
    scans: lists of component indices, one SOS each (default: one interleaved scan); a scan of one component is not
    interleaved.  restart: DRI interval in MCUs (of each scan).  ids: component ids.  jfif: write the APP0 segment.
    adobe: transform byte of an APP14 Adobe segment, or None.  progressive: SOF2 with spectral selection only, every
    scan of `scans` split into a DC scan and one AC scan per component.  between: {scan index: bytes} inserted in
    front of that SOS."""
    app0, _, dht, codes = _tables(90)
    H, W = size
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    comps = []
    for c, (h, v) in enumerate(sampling):
        assert hmax % h == 0 and vmax % v == 0
        b = np.asarray(blocks[c])
        assert b.shape == (mcuy * v, mcux * h, 64), (c, b.shape)
        cw, ch = -(-W * h // hmax), -(-H * v // vmax)  # the component's size in samples
        comps.append(dict(h=h, v=v, tq=0 if c == 0 else 1, tab=0 if c == 0 else 1, cbw=-(-cw // 8), cbh=-(-ch // 8),
                          blocks=b))
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += app0
    if adobe is not None:
        out += segment(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, adobe))
    for t in (0, 1):
        entries = [int(x) for x in qt[t]]
        out += segment(0xDB, bytes([(pq[t] << 4) | t]) + (struct.pack(">64H", *entries) if pq[t] else bytes(entries)))
    out += segment(0xC2 if progressive else 0xC0, struct.pack(">BHHB", 8, H, W, 3) + b"".join(
        bytes([ids[c], (k["h"] << 4) | k["v"], k["tq"]]) for c, k in enumerate(comps)))
    out += dht
    if restart:
        out += segment(0xDD, struct.pack(">H", restart))
    scans = [[0, 1, 2]] if scans is None else scans
    if progressive:  # (components, Ss, Se)
        script = []
        for sc in scans:
            script.append((sc, 0, 0))
            script += [([c], 1, 63) for c in sc]
    else:
        script = [(sc, 0, 63) for sc in scans]
    for si, (sc, ss, se) in enumerate(script):
        if between and si in between:
            out += between[si]
        out += segment(0xDA, bytes([len(sc)]) + b"".join(bytes([ids[c], (comps[c]["tab"] << 4) | comps[c]["tab"]])
                                                         for c in sc) + bytes([ss, se, 0]))
        bits, pred, todo, rst = _Bits(), [0, 0, 0], restart, 0

        def block(c, zz):
            k = comps[c]
            if ss == 0:
                _put_dc(bits, codes[(0, k["tab"])], int(zz[0]) - pred[c])
                pred[c] = int(zz[0])
            if se == 63:
                _put_ac(bits, codes[(1, k["tab"])], zz)

        if len(sc) == 1:
            k = comps[sc[0]]
            units = [[(sc[0], by, bx)] for by in range(k["cbh"]) for bx in range(k["cbw"])]
        else:
            units = [[(c, my * comps[c]["v"] + v, mx * comps[c]["h"] + h) for c in sc
                      for v in range(comps[c]["v"]) for h in range(comps[c]["h"])]
                     for my in range(mcuy) for mx in range(mcux)]
        for unit in units:
            if restart:
                if todo == 0:
                    bits.flush()
                    bits.out += bytes([0xFF, 0xD0 + rst])
                    rst, pred, todo = (rst + 1) & 7, [0, 0, 0], restart
                todo -= 1
            for c, by, bx in unit:
                block(c, comps[c]["blocks"][by, bx])
        bits.flush()
        out += bits.out
    return bytes(out + b"\xff\xd9")


def ycc(rgb) -> np.ndarray:
    """The YCbCr planes of an RGB frame, for write(): the file then shows the frame, not its channels as Y, Cb, Cr."""
    return np.asarray(Image.fromarray(rgb).convert("YCbCr"))


def pil(data: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == "RGB", im.mode
        return np.asarray(im)


@functools.lru_cache(maxsize=None)
def cases():
    """((name, bytes), ...): every sampling of SAMPLINGS at every size of SIZES; RGB-coded 1x1-sampled files both
    ways libjpeg recognises them; the scan scripts on 4:4:4, 4:2:0 and 4:4:0, some with a restart interval (4:2:0
    only at the sizes wider than 4 pixels: below that the decoder hands 4:2:0 back whatever the scans)."""
    out = []
    for si, (h, w) in enumerate(SIZES):
        img = scene(h, w, si)
        for name, (sampling, _, _) in SAMPLINGS.items():
            out.append((f"{name}_{h}x{w}", write(img, sampling)))
        out.append((f"rgb_adobe_{h}x{w}", write(img, S444, jfif=False, adobe=0)))
        out.append((f"rgb_ids_{h}x{w}", write(img, S444, jfif=False, ids=(82, 71, 66))))
        for k, (sname, script) in enumerate(SCAN_SCRIPTS.items()):
            for lname, sampling in (("444", S444), ("420", S420), ("440", S440)):
                if lname == "420" and w <= 4:
                    continue  # 4:2:0 chroma narrower than 3 samples stays handed back, in any number of scans
                restart = 3 if (si + k) % 3 == 0 else 0
                out.append((f"scans_{sname}_{lname}_r{restart}_{h}x{w}",
                            write(img, sampling, scans=script, restart=restart)))
    # a restart interval on the new samplings in one scan, and an RGB-coded file that is subsampled as well
    out.append(("411_r2_37x53", write(scene(37, 53, 40), S411, restart=2)))
    out.append(("440_r1_33x17", write(scene(33, 17, 41), S440, restart=1)))
    out.append(("rgb_adobe_440_17x33", write(scene(17, 33, 42), S440, jfif=False, adobe=0)))
    return tuple(out)


def expected_layout(name):
    """(layout, rh, rv, rgb_coded, multiscan) the parser should report for a case of cases()."""
    key = name.split("_")[0]
    if key == "rgb":
        return (4, 1, 2, True, False) if "_440_" in name else (1, 1, 1, True, False)
    if key == "scans":
        lay = name.split("_")[-3]
        return {"444": (1, 1, 1), "420": (3, 2, 2), "440": (4, 1, 2)}[lay] + (False, True)
    for sname, (_, layout, (rh, rv)) in SAMPLINGS.items():
        if name.startswith(sname + "_"):
            return (layout, rh, rv, False, False)
    raise KeyError(name)


def self_test():
    from inference_arena_amd.ops import native

    C = native()
    for name, data in cases():
        assert pil(data).shape[2] == 3, name
    for si, (h, w) in enumerate(SIZES):
        if w <= 4:
            continue  # narrow fancy chroma: handed back by design
        data = write(scene(h, w, si), S420)
        st, err, rgb = C.jpeg_decode_host(data)
        assert st == "ok", (h, w, err)
        np.testing.assert_array_equal(rgb, pil(data))
    return len(cases())


if __name__ == "__main__":
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    print(f"jpeg_layout_cases: ok ({self_test()} cases)")
