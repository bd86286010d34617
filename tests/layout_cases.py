"""Inputs shared by tests/test_layouts_ref.py (CPU) and tests/test_gpu_layouts.py (GPU).

Every case is built once per process from chosen coefficients (tools/jd_coef.py): the stream, the
plain reference of the same coefficients, and what the coverage audits need.  Nothing here
depends on a decoder's output.
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import jd_coef  # noqa: E402

# (Y, Cb, Cr) factors (h, v); one entry: grayscale
LAYOUTS = {
    "4x1": [(4, 1), (1, 1), (1, 1)],
    "4x2": [(4, 2), (1, 1), (1, 1)],
    "1x4": [(1, 4), (1, 1), (1, 1)],
    "2x4": [(2, 4), (1, 1), (1, 1)],
    "2x1,2x1,1x1": [(2, 1), (2, 1), (1, 1)],
    "2x2,1x2,2x1": [(2, 2), (1, 2), (2, 1)],
    "1x2,1x2,1x1": [(1, 2), (1, 2), (1, 1)],
    "4x1,2x1,1x1": [(4, 1), (2, 1), (1, 1)],
    "2x1,2x1,2x1": [(2, 1), (2, 1), (2, 1)],
    "1x1,2x1,2x1": [(1, 1), (2, 1), (2, 1)],
    "1x1,2x2,1x1": [(1, 1), (2, 2), (1, 1)],
    "4:4:4": [(1, 1), (1, 1), (1, 1)],
    "4:2:2": [(2, 1), (1, 1), (1, 1)],
    "4:2:0": [(2, 2), (1, 1), (1, 1)],
    "4:4:0": [(1, 2), (1, 1), (1, 1)],
    "gray": [(1, 1)],
}
COLOUR_LAYOUTS = ["4:4:4", "4:2:2", "4:2:0", "4:4:0", "4x1", "4x2", "2x2,1x2,2x1", "4x1,2x1,1x1"]
QUANT_LAYOUTS = ["4:2:0", "4:4:4", "4x1,2x1,1x1"]
QUANT_STEPS = [1, 63, 64, 255, 256, 16383, 16384, 32767, 32768, 32769, 65535]
ENTRY_COUNTS = [0, 1, 7, 8, 9, 31, 32, 33, 63]
TILE_BLOCKS = 60  # blocks per IDCT/colour tile (jd_internal.hpp kTileMaxBlocks)

# Annex K.1 (quality 50), natural order; the streams carry them in zig-zag order
_K1_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
            14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
_K1_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
              47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
Q_LUMA = [_K1_LUMA[n] for n in jd_coef.ZIGZAG]
Q_CHROMA = [_K1_CHROMA[n] for n in jd_coef.ZIGZAG]
UNIT = [1] * 64


def geometry(name, mcu_rows=2):
    """(factors, hmax, vmax, blocks per MCU, MCUs per tile, default width, default height)."""
    f = LAYOUTS[name]
    eff = [(1, 1)] if len(f) == 1 else f
    hmax, vmax = max(h for h, _ in eff), max(v for _, v in eff)
    bpm = sum(h * v for h, v in eff)
    tm = TILE_BLOCKS // bpm
    return SimpleNamespace(factors=f, eff=eff, hmax=hmax, vmax=vmax, bpm=bpm, tile_mcus=tm,
                           width=8 * hmax * (tm + 1) - 3, height=8 * vmax * mcu_rows - 1)


def _case(name, tag, width, height, coefs, qtabs, restart=0, **extra):
    f = LAYOUTS[name]
    data = jd_coef.build(width, height, f, coefs, qtabs, restart=restart)
    pl = jd_coef.planes(width, height, f, coefs, qtabs)
    ycc = jd_coef.upsampled(width, height, f, pl)
    return SimpleNamespace(id=f"{name}-{tag}", layout=name, width=width, height=height, factors=f, coefs=coefs,
                           qtabs=qtabs, restart=restart, data=data, ycc=ycc, ref=jd_coef.colour(*ycc), **extra)


def _zeros(width, height, factors):
    return [np.zeros(s, np.int32) for s in jd_coef.coef_shapes(width, height, factors)]


# ---------------------------------------------------------------------------------------------
# a. layout matrix: random dense coefficients
# ---------------------------------------------------------------------------------------------
def _random_coefs(rng, g, width, height):
    """About 30 % non-zero positions.  MCU row 0 keeps every product inside int16 (|AC| <= 100,
    |DC| <= 1024: the packed IDCT form); the others draw AC from +-1023 and DC from +-2047, which
    sends their tiles to the exact form."""
    coefs = _zeros(width, height, g.factors)
    for c, a in enumerate(coefs):
        v = g.eff[c][1]
        for br in range(a.shape[0]):
            big = br // v > 0
            ac = rng.integers(-1023, 1024, a.shape[1:]) if big else rng.integers(-100, 101, a.shape[1:])
            ac *= rng.random(a.shape[1:]) < 0.3
            ac[:, 0] = rng.integers(-2047, 2048, a.shape[1]) if big else rng.integers(-1024, 1025, a.shape[1])
            a[br] = ac
    return coefs


@functools.lru_cache(None)
def matrix_cases():
    out = []
    for i, name in enumerate(LAYOUTS):
        g = geometry(name)
        rng = np.random.default_rng(1000 + i)
        odd = next(r for r in range(2, 64) if g.tile_mcus % r)  # no divisor of the tile's MCU count
        qt = [Q_LUMA, Q_CHROMA]
        out.append(_case(name, "5x3", 5, 3, _random_coefs(rng, g, 5, 3), qt))
        for restart in (0, 1, odd):
            out.append(_case(name, f"rst{restart}", g.width, g.height, _random_coefs(rng, g, g.width, g.height), qt,
                             restart=restart))
    return out


# ---------------------------------------------------------------------------------------------
# b. colour stage, directed
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def exact_pairs():
    """The (Cb, Cr) pairs of [-256, 255]^2 that take the double-precision G path."""
    cb, cr = np.meshgrid(np.arange(-256, 256), np.arange(-256, 256), indexing="ij")
    m = jd_coef.exact_class(cb, cr)
    return list(zip(cb[m].tolist(), cr[m].tolist()))


def _dc_of(sample):
    """DC (unit quant, no AC) whose block is flat at `sample`: (dc + 4) >> 3, within +-2047."""
    return max(-2047, 8 * sample)


def _ramp_block(kind, target, level):
    """Cr block (zig-zag, unit quant) ramping through `level`: kind 'h' puts it in column `target`,
    'v' in row `target`, 'd' on the anti-diagonal.  The DC is searched so that the IDCT output
    hits `level` exactly there."""
    import jdoracle

    amp = 60 if level <= 0 else -60  # ramp away from the clip limit
    cands = []
    for d in range(8 * level - 100, 8 * level + 101):
        zz = np.zeros(64, np.int32)
        zz[0] = d
        if kind in ("h", "d"):
            zz[1] = amp
        if kind in ("v", "d"):
            zz[2] = amp
        cands.append(zz)
    px = jdoracle.idct(np.stack(cands)).reshape(-1, 8, 8)
    if kind == "h":
        hit = (px[:, :, target] == level).sum(1)
    elif kind == "v":
        hit = (px[:, target, :] == level).sum(1)
    else:
        hit = (px[:, np.arange(8), 7 - np.arange(8)] == level).sum(1)
    ok = (np.abs(np.array([c[0] for c in cands])) <= 2047)
    best = int(np.argmax(hit * ok))
    return cands[best]


_ramp_block = functools.lru_cache(None)(_ramp_block)


def _colour_coefs(name, width, height, seed):
    g = geometry(name)
    rng = np.random.default_rng(seed)
    coefs = _zeros(width, height, g.factors)
    pairs = exact_pairs()
    _, _, mcux, mcuy = jd_coef.grid(width, height, g.factors)
    # Y: random AC on DCs of +-2047 and 0 (spans both clip limits, varies per pixel), and DC-only
    # blocks at -256 and 255
    y = coefs[0]
    n = 0
    for br in range(y.shape[0]):
        for bc in range(y.shape[1]):
            n += 1
            if n % 7 == 0:
                y[br, bc, 0] = -2047 if (n // 7) % 2 else 2040
                continue
            y[br, bc, 0] = (-2047, 2047, 0)[rng.integers(0, 3)]
            ac = rng.integers(-120, 121, 63)
            y[br, bc, 1:] = ac * (rng.random(63) < 0.15)
    # chroma, per MCU: flat at an exact-class pair / Cb flat and Cr ramping through the pair's Cr
    # (some pixels of a group exact-class, others not) / both at the clip limits
    kinds = ("flat", "h", "d", "sat", "v", "h", "flat", "d")
    t = {"h": 0, "v": 0, "d": 0}  # ramp targets: every column / row in turn
    for m in range(mcux * mcuy):
        my, mx = divmod(m, mcux)
        kind = kinds[(m + my) % len(kinds)]
        cb0, cr0 = pairs[(5 * m + 3) % len(pairs)]
        for c in (1, 2):
            h, v = g.eff[c]
            for by in range(v):
                for bx in range(h):
                    blk = coefs[c][my * v + by, mx * h + bx]
                    if kind == "sat":
                        blk[0] = (-2047, 2040)[((m // 8) >> (c - 1)) & 1]
                    elif c == 1 or kind == "flat":
                        blk[0] = _dc_of(cb0 if c == 1 else cr0)
                    else:
                        blk[:] = _ramp_block(kind, t[kind] % 8, cr0)
                        t[kind] += 1
    return coefs


def group_audit(ex, rows=None, band=None):
    """Per pixel position j of an 8-pixel group: (exact-class in a group whose other positions are
    not all exact-class, non-exact in a group that has an exact-class pixel).  ex: bool [H, W];
    rows/band: only rows y with y % band in rows."""
    h, w = ex.shape
    n = w // 8  # whole groups (a partial last group lacks some positions)
    gr = ex[:, :8 * n].reshape(h, n, 8)
    if rows is not None:
        gr = gr[[y for y in range(h) if y % band in rows]]
    gr = gr.reshape(-1, 8)
    cnt = gr.sum(1)
    a = [bool((gr[:, j] & (cnt - gr[:, j] < 7)).any()) for j in range(8)]
    b = [bool((~gr[:, j] & (cnt > 0)).any()) for j in range(8)]
    return a, b


def cell_audit(case, mcu_h):
    """Per cell (x mod 8, y mod MCU height): has an exact-class pixel; has each channel at 0 and
    at 255.  Returns the list of failing (what, x, y)."""
    ex = jd_coef.exact_class(case.ycc[1], case.ycc[2])
    ys = np.arange(case.height)[:, None] % mcu_h
    xs = np.arange(case.width)[None, :] % 8
    bad = []
    for cy in range(mcu_h):
        for cx in range(8):
            cell = (ys == cy) & (xs == cx)
            if not (ex & cell).any():
                bad.append(("exact", cx, cy))
            for ch in range(3):
                for lim in (0, 255):
                    if not ((case.ref[..., ch] == lim) & cell).any():
                        bad.append((f"ch{ch}={lim}", cx, cy))
    return bad


# widths of the directed images: the default width's last group varied so that W mod 8 takes 1, 3,
# 4 and 7 (store24 / store12 tails of 1 .. 7 pixels at every byte alignment); heights odd
_COLOUR_TRIM = {"4:4:4": 7, "4:2:2": 5, "4:2:0": 4, "4:4:0": 1, "4x1": 7, "4x2": 5, "2x2,1x2,2x1": 4, "4x1,2x1,1x1": 1}
# MCU rows per directed image: the fewest (>= 2) with which the coverage audits of
# tests/test_layouts_ref.py hold (layouts with few MCUs per row need more rows)
_COLOUR_ROWS = {"4:4:4": 2, "4:2:2": 2, "4:2:0": 2, "4:4:0": 2, "4x1": 2, "4x2": 2, "2x2,1x2,2x1": 2, "4x1,2x1,1x1": 2}


@functools.lru_cache(None)
def colour_cases():
    out = []
    for i, name in enumerate(COLOUR_LAYOUTS):
        g = geometry(name, _COLOUR_ROWS[name])
        width = g.width + 3 - _COLOUR_TRIM[name]
        out.append(_case(name, "colour", width, g.height, _colour_coefs(name, width, g.height, 2000 + i), [UNIT, UNIT]))
    return out


# ---------------------------------------------------------------------------------------------
# c. quantisation range
# ---------------------------------------------------------------------------------------------
# zig-zag positions: first, two middle ones (natural 21 in row 2, natural 56 in row 7), last (row 7)
QUANT_POS = [1, 30, 35, 63]


def fast_k(qmax):
    """The k of the host plan's range test: the fast IDCT form takes -2^(k-1) <= c < 2^(k-1),
    the largest k <= 16 with 2^(k-1) * qmax < 2^15 (0: only c = 0)."""
    k = 0
    while k < 16 and (1 << k) * qmax < 32768:
        k += 1
    return k


def quant_values(qmax):
    """(in-range, out-of-range) AC values around the range test's edge, the 10-bit entry slots'
    escape edge and the Huffman tables' largest size; (in, out) DC values around +-2^15 / qmax."""
    k = fast_k(qmax)
    vals = {-1, 1, 511, -511, 512, -512, 513, -513, 1023, -1023}
    if k >= 1:
        e = 1 << (k - 1)
        vals |= {-e, -e - 1, e - 1, e}
    vals = sorted(v for v in vals if v and abs(v) <= 1023)
    fits = [v for v in vals if -32768 <= v * qmax <= 32767]
    # the test is a power-of-two one: it is exact at the edge values and conservative elsewhere
    ac_in = [v for v in fits if k >= 1 and -(1 << (k - 1)) <= v < (1 << (k - 1))]
    ac_out = [v for v in vals if v not in fits]
    hi, lo = 32767 // qmax, -(32768 // qmax)
    dc_in = [d for d in (hi, lo) if abs(d) <= 2047]
    dc_out = [d for d in (hi + 1, lo - 1) if abs(d) <= 2047]
    return SimpleNamespace(k=k, ac_in=ac_in, ac_mid=[v for v in fits if v not in ac_in], ac_out=ac_out,
                           dc_in=dc_in, dc_out=dc_out)


def _quant_case(name, qmax):
    g = geometry(name)
    qv = quant_values(qmax)
    # One MCU row per out-of-range block: the row's first tile holds that block alone (the exact
    # IDCT form), its second tile none (the fast form); row 0 has none at all.  The values next to
    # the range test's edge and the DCs are alone in their block (a value wrongly let through
    # shows); the others, far outside, share blocks four at a time.  That makes these images
    # taller than the matrix's (up to 8 MCU rows), still a few thousand pixels.
    far = qv.ac_out + qv.ac_mid
    edge = [v for v in far if v in ((-1, 1) if qv.k == 0 else (-(1 << (qv.k - 1)) - 1, 1 << (qv.k - 1)))]
    far = [v for v in far if v not in edge]
    outs = [("dc", d) for d in qv.dc_out] + [("ac", [v]) for v in edge]
    outs += [("ac", far[i:i + 4]) for i in range(0, len(far), 4)]
    rows = 1 + len(outs)
    width, height = g.width, 8 * g.vmax * rows - 1
    coefs = _zeros(width, height, g.factors)
    qy = [qmax] * 64
    qc = [max(1, (qmax + 1) // 2)] * 64
    for p in [0] + QUANT_POS:
        qc[p] = qmax
    rng = np.random.default_rng(3000 + qmax)
    dcs = qv.dc_in + [0]
    for c, a in enumerate(coefs):
        for br in range(a.shape[0]):
            for bc in range(a.shape[1]):
                a[br, bc, 0] = dcs[rng.integers(0, len(dcs))]
                for p in QUANT_POS:
                    if qv.ac_in and rng.random() < 0.5:
                        a[br, bc, p] = qv.ac_in[rng.integers(0, len(qv.ac_in))]
                if (br + bc) % 3 == 0:  # row 7 of the natural order empty in a third of the blocks
                    a[br, bc, 35] = a[br, bc, 63] = 0
    _, _, mcux, _ = jd_coef.grid(width, height, g.factors)
    for r, (what, v) in enumerate(outs, start=1):
        mx = (3 * r) % g.tile_mcus  # an MCU of the row's first tile
        b = (r * 7) % g.bpm         # block of that MCU, in scan order
        c = 0
        while b >= g.eff[c][0] * g.eff[c][1]:
            b -= g.eff[c][0] * g.eff[c][1]
            c += 1
        h, vv = g.eff[c]
        blk = coefs[c][r * vv + b // h, mx * h + b % h]
        if what == "dc":
            blk[0] = v
        else:
            for i, x in enumerate(v):
                blk[QUANT_POS[(r + i) % len(QUANT_POS)]] = x
    return _case(name, f"q{qmax}", width, height, coefs, [qy, qc], qmax=qmax, qv=qv)


@functools.lru_cache(None)
def quant_cases():
    return [_quant_case(name, q) for name in QUANT_LAYOUTS for q in QUANT_STEPS]


# ---------------------------------------------------------------------------------------------
# d. blocks with many entries
# ---------------------------------------------------------------------------------------------
def _entry_case(name, wide, seed):
    g = geometry(name, 3)
    rng = np.random.default_rng(seed)
    coefs = _zeros(g.width, g.height, g.factors)
    _, _, mcux, mcuy = jd_coef.grid(g.width, g.height, g.factors)
    counts = []
    i = 0
    for m in range(mcux * mcuy):  # scan order, so that the running entry count is the decoder's
        my, mx = divmod(m, mcux)
        for c, (h, v) in enumerate(g.eff):
            for by in range(v):
                for bx in range(h):
                    # a spacer block of 0 .. 7 entries, then a listed count: 8 and 9 are coprime,
                    # so every count follows every spacer and starts at every offset mod 8
                    j = i // 2
                    n = (3 * j + j // 8) % 8 if i % 2 == 0 else ENTRY_COUNTS[j % len(ENTRY_COUNTS)]
                    i += 1
                    blk = coefs[c][my * v + by, mx * h + bx]
                    blk[0] = rng.integers(-300, 301)
                    pos = 1 + rng.permutation(63)[:n]
                    val = rng.integers(1, 40, n) * rng.choice([-1, 1], n)
                    if wide and n in (9, 33) and rng.random() < 0.5:
                        val[0] = 700 * rng.choice([-1, 1])  # beyond a 10-bit slot: escaped entry
                    blk[pos] = val
                    counts.append(n)
    return _case(name, "entries-wide" if wide else "entries", g.width, g.height, coefs, [UNIT, [2] * 64],
                 restart=0, counts=counts)


@functools.lru_cache(None)
def entry_cases():
    return [_entry_case(name, wide, 4000 + 2 * i + wide)
            for i, name in enumerate(["4:2:0", "4:4:4", "2x2,1x2,2x1"]) for wide in (0, 1)]


def all_cases():
    return matrix_cases() + colour_cases() + quant_cases() + entry_cases()


@functools.lru_cache(None)
def oracle_outputs(fancy=False):
    """id -> (status, pixels) of jdoracle.decode for every case, computed once per process."""
    import jdoracle

    return {c.id: jdoracle.decode(c.data, fancy=fancy) for c in (matrix_cases() if fancy else all_cases())}
