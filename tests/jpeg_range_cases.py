"""JPEG files with crafted coefficients, for the range tests (test_jpeg_range.py, test_jpeg_range_gpu.py).

A valid baseline file can carry any coefficients its Huffman tables can code, with any quantiser; files encoded from
pixels stay in a narrow range.  The split decoder reconstructs a block only when S = sum |c_k| * q_k is at most
kCoefRangeLimit (csrc/kernels/jpeg_math.h, where the proof is): within it exact arithmetic, the kernels' int32
arithmetic and the 16-bit lanes of libjpeg-turbo's SIMD IDCT agree.  The files here sit on both sides of that limit:

* inside(): must decode natively, status "ok", and equal PIL;
* outside(): must come back "unsupported" from both decode functions, and PIL's pixels differ from what the
  decoder's arithmetic would have made of them (which is why they are handed back).

The files come from jpeg_layout_cases.write_coefs (Huffman tables read from a file PIL writes at run time, so DC
differences stay within +-2047 and AC coefficients within +-1023) and, for the extreme real images, from PIL's own
encoder.  The pixel oracle of every file is PIL's decode of it; a file PIL refuses would be dropped from the lists
(PIL 12.2 with libjpeg-turbo refuses none of them).

port_rgb() is a numpy port of csrc/kernels/jpeg_math.h over the blocks a case was written from, with int32 or int64
accumulators: the decoder's arithmetic without its range check, so that it can be put next to PIL on the outside
files too."""
from __future__ import annotations

import functools
import io
import re
from pathlib import Path
from typing import NamedTuple

import numpy as np
from PIL import Image

import jpeg_layout_cases as L

S422 = [(2, 1), (1, 1), (1, 1)]


@functools.lru_cache(maxsize=None)
def limit() -> int:
    """kCoefRangeLimit, read from the header that defines it."""
    text = (Path(__file__).resolve().parents[1] / "csrc" / "kernels" / "jpeg_math.h").read_text()
    return int(re.search(r"constexpr int32_t kCoefRangeLimit = (\d+);", text).group(1))


class Case(NamedTuple):
    name: str
    data: bytes
    size: tuple          # (H, W)
    sampling: list
    blocks: list | None  # per component int[bh][bw][64], zigzag order, as written; None for a PIL-encoded file
    qt: dict | None      # {0: luma, 1: chroma} zigzag order


_NAT_OF_ZZ = np.array(L._ZIGZAG)           # zigzag index -> natural index
_ZZ_OF_NAT = np.argsort(_NAT_OF_ZZ)        # natural index -> zigzag index


def zz(row, col):
    return int(_ZZ_OF_NAT[row * 8 + col])


def block_sums(blocks, q):
    """S of every block of one component."""
    return (np.abs(np.asarray(blocks, np.int64)) * np.asarray(q, np.int64)).sum(-1)


def worst_sum(case) -> int:
    return max(int(block_sums(b, case.qt[0 if c == 0 else 1]).max()) for c, b in enumerate(case.blocks))


# ---- numpy port of csrc/kernels/jpeg_math.h --------------------------------------------------------------------

_F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137,
          f1961=16069, f2053=16819, f2562=20995, f3072=25172)


def idct8(x, shift):
    """jpegm::idct8 along the last axis of an int32 or int64 array (int32 wraps as the C++ does on two's complement)."""
    T = x.dtype.type
    k = {n: T(v) for n, v in _F.items()}
    i = [x[..., j] for j in range(8)]
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * k["f0541"]
    tmp2 = z1 - z3 * k["f1847"]
    tmp3 = z1 + z2 * k["f0765"]
    tmp0 = (i[0] + i[4]) * T(1 << 13)
    tmp1 = (i[0] - i[4]) * T(1 << 13)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * k["f1175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * k["f0298"], tmp1 * k["f2053"], tmp2 * k["f3072"], tmp3 * k["f1501"]
    z1, z2 = -(z1 * k["f0899"]), -(z2 * k["f2562"])
    z3, z4 = z5 - z3 * k["f1961"], z5 - z4 * k["f0390"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
           tmp10 - tmp3]
    return np.stack([(o + T(1 << (shift - 1))) >> T(shift) for o in out], -1)


def port_plane(blocks, q, dtype):
    """The sample plane of one component: blocks int[bh][bw][64] in zigzag order as the file codes them."""
    b = np.asarray(blocks).astype(np.int16)  # the decoder stores int16: a DC predictor beyond it wraps
    bh, bw = b.shape[:2]
    nat = np.zeros((bh, bw, 64), dtype)
    with np.errstate(over="ignore"):
        nat[:, :, _NAT_OF_ZZ] = b.astype(dtype) * np.asarray(q).astype(np.uint16).astype(dtype)
        a = nat.reshape(bh, bw, 8, 8)                                # [row][col]
        ws = idct8(np.swapaxes(a, -1, -2), 11)                       # pass 1 over every column: [col][row]
        o = idct8(np.ascontiguousarray(np.swapaxes(ws, -1, -2)), 18)  # pass 2 over every row
    px = np.clip(o.astype(np.int64) + 128, 0, 255)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def port_rgb(case, dtype=np.int32):
    """The RGB frame jpeg_coefs_to_rgb / the kernels compute from the case's blocks (4:4:4, 4:2:2, 4:2:0; YCbCr)."""
    H, W = case.size
    planes = [port_plane(b, case.qt[0 if c == 0 else 1], dtype) for c, b in enumerate(case.blocks)]
    rh, rv = case.sampling[0]
    y, x = np.mgrid[0:H, 0:W]
    yy = planes[0][y, x]
    cc = []
    for p in planes[1:]:
        cw, ch = -(-W // rh), -(-H // rv)
        cx, cy = x // rh, y // rv
        nx = np.where(x & 1, np.minimum(cx + 1, cw - 1), np.maximum(cx - 1, 0))
        ny = np.where(y & 1, np.minimum(cy + 1, ch - 1), np.maximum(cy - 1, 0))
        if (rh, rv) == (1, 1):
            cc.append(p[y, x])
        elif (rh, rv) == (2, 1):   # fancy_h2v1
            cc.append((p[y, cx] * 3 + p[y, nx] + np.where(x & 1, 2, 1)) >> 2)
        elif (rh, rv) == (2, 2):   # fancy_h2v2
            this, other = p[cy, cx] * 3 + p[ny, cx], p[cy, nx] * 3 + p[ny, nx]
            cc.append((this * 3 + other + np.where(x & 1, 7, 8)) >> 4)
        else:
            raise NotImplementedError(case.sampling)
    cb, cr = cc[0] - 128, cc[1] - 128   # ycc_to_rgb
    r = yy + ((91881 * cr + 32768) >> 16)
    g = yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = yy + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def pil_or_none(data):
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im.convert("RGB"))
    except Exception:  # noqa: BLE001
        return None


# ---- crafted blocks --------------------------------------------------------------------------------------------

KINDS = ("dense", "sparse", "cols04", "cols04_row")


def _support(kind, rng):
    """Zigzag indices a block of this kind may load."""
    if kind == "dense":
        nat = np.arange(64)
    elif kind == "sparse":
        nat = rng.choice(64, size=int(rng.integers(1, 6)), replace=False)
    else:
        nat = np.array([r * 8 + c for r in range(8) for c in (0, 4)])
        if kind == "cols04_row":
            nat = np.union1d(nat, int(rng.integers(0, 8)) * 8 + np.arange(8))
    return _ZZ_OF_NAT[nat]


def scaled_block(kind, q, target, rng):
    """A random block of `kind` whose S is as close below `target` as its quantisers allow: the random pattern is
    scaled down to the target, then topped up one step at a time wherever a step still fits."""
    sup = _support(kind, rng)
    w = rng.normal(0, 1, len(sup)) * rng.choice([0.1, 1.0, 4.0], len(sup))
    sign = np.where(w < 0, -1, 1)
    mag = np.floor(np.abs(w) * target / (np.abs(w) * q[sup]).sum()).astype(np.int64)
    left = target - int((mag * q[sup]).sum())
    for j in rng.permutation(len(sup)):
        n = left // int(q[sup[j]])
        mag[j] += n
        left -= n * int(q[sup[j]])
    blk = np.zeros(64, np.int64)
    blk[sup] = sign * mag
    assert target - int(q[sup].min()) < int((np.abs(blk) * q).sum()) <= target
    return blk


def _random_q(rng):
    # >= 6, so that S <= limit keeps every coefficient within +-1023 and every DC difference within +-2047
    return {0: rng.integers(6, 41, 64), 1: rng.integers(6, 41, 64)}


def _coef_case(name, size, sampling, blocks, qt, **kw):
    return Case(name, L.write_coefs(size, blocks, qt, sampling, **kw), size, sampling, blocks, qt)


def _shape(size, sampling):
    """Block grid (rows, cols) of each component."""
    H, W = size
    hmax, vmax = sampling[0]
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    return [(mcuy * v, mcux * h) for h, v in sampling]


def _luma_only(name, size, luma, q, **kw):
    """A 4:4:4 file with the given luma blocks (row by row) and Cb = Cr = 128."""
    shp = _shape(size, L.S444)
    blocks = [np.asarray(luma, np.int64).reshape(shp[0] + (64,)), np.zeros(shp[1] + (64,), np.int64),
              np.zeros(shp[2] + (64,), np.int64)]
    return _coef_case(name, size, L.S444, blocks, {0: np.asarray(q), 1: np.full(64, 16)}, **kw)


def _one(entries):
    blk = np.zeros(64, np.int64)
    for k, v in entries.items():
        blk[k] = v
    return blk


def _random_cases():
    """Random blocks of the four kinds just under the limit, in every component: per kind three 64x64 4:4:4 files
    (192 blocks each) and three 64x64 4:2:0 files (96 blocks each), 864 blocks per kind."""
    out = []
    for ki, kind in enumerate(KINDS):
        for li, (lname, sampling) in enumerate((("444", L.S444), ("420", L.S420))):
            for f in range(3):
                rng = np.random.default_rng([2024, ki, li, f])
                qt = _random_q(rng) if f else {t: L._tables(50)[1][t].astype(np.int64) for t in (0, 1)}
                blocks = [np.array([[scaled_block(kind, qt[0 if c == 0 else 1], limit(), rng) for _ in range(bw)]
                                    for _ in range(bh)]) for c, (bh, bw) in enumerate(_shape((64, 64), sampling))]
                out.append(_coef_case(f"random_{kind}_{lname}_{f}", (64, 64), sampling, blocks, qt))
    return out


def _by_dc(blocks):
    """Ordered by DC, so that every DC difference of the scan stays small."""
    return sorted(blocks, key=lambda b: int(b[0]))


def _at_limit_cases():
    """Blocks whose S is exactly the limit, in the patterns that load the 16-bit lanes most.

    at_limit_single: one coefficient of +-1 against a 16-bit quantiser equal to the limit: the DC alone (the
    shortcut's shift of a block without AC), a coefficient in row 0 (no AC in any column either), and one in every
    other row and column class.  at_limit_pairs: 8-bit quantiser d (a small divisor of the limit) everywhere and two
    coefficients that share limit / d: rows 0 and 4, 7 and 3, 5 and 1 of a column (pass 1's pair sums and difference)
    and columns 0 and 4, 7 and 3, 5 and 1 of row 1, the row with the largest pass-1 gain (pass 2's pair sums), with
    equal and opposite signs, and once next to a DC."""
    lim = limit()
    single = []
    for s in (1, -1):
        single += [_one({0: s}), _one({zz(0, 1): s}), _one({zz(0, 7): s}), _one({zz(1, 0): s}), _one({zz(1, 4): s}),
                   _one({zz(4, 0): s}), _one({zz(7, 7): s}), _one({zz(3, 5): s})]
    d = next(k for k in range(3, 256) if lim % k == 0 and lim // k <= 2046)
    a, b = lim // d // 2, lim // d - lim // d // 2
    pairs = []
    for s in (1, -1):
        pairs += [_one({zz(0, 3): s * a, zz(4, 3): s * b}), _one({zz(0, 5): s * a, zz(4, 5): -s * b}),
                  _one({zz(7, 2): s * a, zz(3, 2): s * b}), _one({zz(5, 6): s * a, zz(1, 6): s * b}),
                  _one({zz(1, 0): s * a, zz(1, 4): s * b}), _one({zz(1, 0): s * b, zz(1, 4): -s * a}),
                  _one({zz(1, 7): s * a, zz(1, 3): s * b}), _one({zz(1, 5): s * a, zz(1, 1): s * b}),
                  _one({zz(7, 0): s * a, zz(7, 4): s * b}), _one({zz(1, 0): s * (a - 8), zz(1, 4): s * b, 0: s * 8}),
                  _one({0: s * a, zz(4, 0): s * b}), _one({0: s * (lim // d)})]
    out = []
    for name, pats, q, pq in (("at_limit_single", single, np.full(64, lim), (1, 1)),
                              ("at_limit_pairs", pairs, np.full(64, d), (0, 0))):
        grid = np.array(_by_dc(pats)).reshape(len(pats) // 8, 8, 64)
        case = _coef_case(name, (8 * grid.shape[0], 8 * grid.shape[1]), L.S444, [grid, grid, grid], {0: q, 1: q}, pq=pq)
        assert all((block_sums(bk, q) == lim).all() for bk in case.blocks)
        out.append(case)
    # columns 0 and 4 of row 1 again, as +-1 against 16-bit quantisers that share the limit (and, in outside(),
    # the limit + 1)
    out.append(_row1_pair("at_limit_row1_pq1", lim))
    return out


def _row1_pair(name, total):
    q = np.full(64, 16)
    q[zz(1, 0)], q[zz(1, 4)] = total // 2, total - total // 2
    luma = [_one({zz(1, 0): s, zz(1, 4): t}) for s in (1, -1) for t in (1, -1)]
    case = _luma_only(name, (8, 32), luma, q, pq=(1, 0))
    assert worst_sum(case) == total
    return case


def _clamp_cases():
    """Y in {0, 255} against Cb, Cr in {0, 255}, as DC-only blocks (q = 8: the sample is 128 + DC): all eight
    combinations, one per MCU, which drives ycc_to_rgb's three clamps to both sides; with subsampled chroma the fancy
    filters blend neighbouring MCUs on top."""
    out = []
    q = {0: np.full(64, 8), 1: np.full(64, 8)}
    dc = {0: -128, 255: 127}
    for lname, sampling, size in (("444", L.S444, (8, 64)), ("422", S422, (16, 64)), ("420", L.S420, (32, 64))):
        shp = _shape(size, sampling)
        blocks = [np.zeros(s + (64,), np.int64) for s in shp]
        mcus = [(my, mx) for my in range(shp[1][0]) for mx in range(shp[1][1])]
        assert len(mcus) == 8
        for i, (my, mx) in enumerate(mcus):
            h, v = sampling[0]
            blocks[0][my * v:(my + 1) * v, mx * h:(mx + 1) * h, 0] = dc[255 * (i & 1)]
            blocks[1][my, mx, 0] = dc[255 * (i >> 1 & 1)]
            blocks[2][my, mx, 0] = dc[255 * (i >> 2 & 1)]
        out.append(_coef_case(f"clamps_{lname}", size, sampling, blocks, q))
    return out


def _pq1_cases():
    """16-bit quantisation tables (DQT precision 1): one with entries an 8-bit table could hold, one with entries of
    a few thousand against coefficients of +-1 and 0."""
    rng = np.random.default_rng(77)
    small = _random_q(rng)
    blocks = [np.array([[scaled_block("dense", small[0 if c == 0 else 1], 3000, rng) for _ in range(4)]
                        for _ in range(2)]) for c in range(3)]
    out = [_coef_case("pq1_small_entries", (16, 32), L.S444, blocks, small, pq=(1, 1))]
    big = {0: rng.integers(2000, 5001, 64), 1: rng.integers(2000, 5001, 64)}
    blocks = []
    for c in range(3):
        b = np.zeros((2, 4, 64), np.int64)
        for by in range(2):
            for bx in range(4):
                b[by, bx, int(rng.integers(0, 64))] = int(rng.choice([-1, 1]))
        blocks.append(b)
    out.append(_coef_case("pq1_entries_of_thousands", (16, 32), L.S444, blocks, big, pq=(1, 1)))
    return out


EXTREME_QUALITIES = (1, 10, 50, 95, 100)


def extreme_images():
    """{name: 64x64 RGB}: contents whose blocks carry the most DCT energy an 8-bit image can.  "noise_grey" (the same
    0 / 255 noise in all three channels, so that luma takes all of it) is the one content whose blocks pass the
    limit, at every quality (S up to about 7000): it is not among inside() but in beyond().  Other full-swing noise and
    dither in luma would join it; these seven contents are not a survey of what pixels can do."""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:64, 0:64]
    grey = lambda m: np.repeat((m.astype(np.uint8) * 255)[:, :, None], 3, 2)  # noqa: E731
    stripes = np.zeros((64, 64, 3), np.uint8)
    for i, colour in enumerate([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),
                                (0, 0, 0), (255, 255, 255)]):
        stripes[:, i::8] = colour
    return {
        "noise": (rng.integers(0, 2, (64, 64, 3)) * 255).astype(np.uint8),
        "noise_grey": grey(rng.integers(0, 2, (64, 64))),
        "checker1": grey((x + y) & 1),
        "checker2": grey(((x >> 1) + (y >> 1)) & 1),
        "rows1": grey(y & 1),
        "one_lit": grey(((x & 7) == 3) & ((y & 7) == 5)),
        "stripes": stripes,
    }


def _extreme_cases(beyond=False):
    out = []
    for name, img in extreme_images().items():
        if (name == "noise_grey") != beyond:
            continue
        for quality in EXTREME_QUALITIES:
            for sub in (0, 2):
                b = io.BytesIO()
                Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling=sub)
                out.append(Case(f"extreme_{name}_q{quality}_s{sub}", b.getvalue(), (64, 64),
                                L.S444 if sub == 0 else L.S420, None, None))
    return out


@functools.lru_cache(maxsize=None)
def inside():
    """Cases the decoder must take: S <= limit in every block (crafted), or PIL-encoded from pixels."""
    out = _random_cases() + _at_limit_cases() + _clamp_cases() + _pq1_cases()
    assert all(worst_sum(c) <= limit() for c in out)
    out += _extreme_cases()
    return tuple(c for c in out if pil_or_none(c.data) is not None)


def with_blocks(case, coefs):
    """A PIL-encoded case with the blocks the decoder read from it (`coefs`: what the jpeg_coefs binding returns, which
    carries the coefficients of a handed-back baseline file too) and the tables of its DQT segments, for port_rgb()."""
    qt = {}
    for m, a, e in L.segments(case.data):
        seg, q = case.data[a + 4:e], 0
        while m == 0xDB and q < len(seg):
            assert seg[q] >> 4 == 0
            qt[seg[q] & 15] = np.frombuffer(seg[q + 1:q + 65], np.uint8).astype(np.int64)
            q += 65
    blocks = []
    for comp in coefs["comps"]:
        n = comp["bw"] * comp["bh"] * 64
        blk = coefs["coef"][comp["coef_off"]:comp["coef_off"] + n].reshape(comp["bh"], comp["bw"], 64)
        blocks.append(blk[:, :, _NAT_OF_ZZ].astype(np.int64))
    return case._replace(blocks=blocks, qt=qt)


@functools.lru_cache(maxsize=None)
def beyond():
    """PIL-encoded images the criterion turns away although they come from pixels: handed back, not wrong."""
    return tuple(_extreme_cases(beyond=True))


@functools.lru_cache(maxsize=None)
def outside():
    """Cases the decoder must hand back: some block has S > limit, and PIL's 16-bit lanes do wrap on it.  Luma only
    (Cb = Cr = 128), 4:4:4."""
    lim = limit()
    rng = np.random.default_rng(11)
    out = []
    # dense noise +-100 against q = 16
    out.append(_luma_only("dense_noise_100_q16", (16, 32), rng.integers(-100, 101, (8, 64)), np.full(64, 16)))
    # one AC coefficient of +-1023 against q = 255, two blocks
    out.append(_luma_only("ac_1023_q255", (8, 16), [_one({zz(2, 3): 1023}), _one({zz(5, 1): -1023})], np.full(64, 255)))
    # a DC chain whose dequantised values run from 16 000 to 32 640 in steps the DC table can code
    out.append(_luma_only("dc_chain_q16", (8, 40), [_one({0: v}) for v in (1000, 1260, 1520, 1780, 2040)],
                          np.full(64, 16)))
    # DC steps of +2047 until the predictor has left int16 (the 17th block), q = 1
    out.append(_luma_only("dc_predictor_past_int16", (24, 48), [_one({0: 2047 * (i + 1)}) for i in range(18)],
                          np.ones(64, np.int64)))
    # one coefficient in row 0 with |c * q| >= 8192: the shortcut for columns without AC shifts it in 16 bits
    out.append(_luma_only("row0_shortcut_shift", (8, 16), [_one({zz(0, 1): 100}), _one({zz(0, 6): -90})],
                          np.full(64, 100)))
    # columns 0 and 4 loaded to 9000 <= S < 16 000: row 1 twice (pass 2's pair sum wraps for certain), then random
    q = np.full(64, 10)
    luma = [_one({zz(1, 0): 450, zz(1, 4): 450}), _one({zz(1, 0): -700, zz(1, 4): -800})]
    luma += [scaled_block("cols04", q, int(t), rng) for t in rng.integers(9000, 16000, 6)]
    case = _luma_only("cols04_9000_16000", (8, 64), _by_dc(luma), q)
    assert all(9000 <= s < 16000 for s in block_sums(case.blocks[0], q).ravel())
    out.append(case)
    # a 16-bit quantiser of 40 000 against +-1
    q = np.full(64, 16)
    q[zz(2, 2)] = 40000
    out.append(_luma_only("pq1_entry_40000", (8, 16), [_one({zz(2, 2): 1}), _one({zz(2, 2): -1})], q, pq=(1, 0)))
    # the limit + 1, in the pattern that reaches pass 2's 16-bit pair sum first
    out.append(_row1_pair("limit_plus_1", lim + 1))
    assert all(worst_sum(c) > lim for c in out)
    return tuple(c for c in out if pil_or_none(c.data) is not None)
