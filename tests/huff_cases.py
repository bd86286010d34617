"""Inputs shared by tests/test_huff_ref.py (CPU) and tests/test_gpu_huff.py (GPU): the Huffman
table space.

Every case is built once per process by tools/jd_coef.py from chosen coefficients (or, for the
symbol-level cases, chosen symbols) and a chosen table set: the stream, its entropy-coded bit
count and the plain reference of the same coefficients (which never sees the tables).  Nothing
here depends on a decoder's output.  The families (what each must make happen is asserted by the
audits of tests/test_huff_ref.py):

  stair    DC symbols 0..16 and all 256 AC symbols, codes of every length 2..16 (1..16 in the luma
           AC table): every arm of the slow path's limit count, every size behind long codes
  edge     codes of 9, 10 and 11 bits, l + size = 10 exactly, size 9 against 10 behind a 1-bit code,
           DC sizes 11 and 12 behind short codes
  uniform  every code of 10 bits / of 11 bits / of 15 and 16 bits (no self-synchronisation)
  pairs    1-3-bit codes, so that most index entries hold two symbols; second symbols of every
           size 1..8 (size 8 needs the complete two-symbol code {ZRL: 0, 0x08: 1})
  dense    table sets whose densest block takes 2, 3, .. 8 walk bits per region word
  six      six (and five) distinct tables in one frame, permuted DHT ids, every DHT packing, an AC
           table whose bytes equal a DC table's
  ident    table sets that differ in the values' order only / in the counts only / in the class
           (DC or AC) of a table of the same bytes
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

LAYOUTS = {"gray": [(1, 1)], "4:4:4": [(1, 1), (1, 1), (1, 1)], "4:2:0": [(2, 2), (1, 1), (1, 1)]}
TILE_BLOCKS = 60  # blocks per IDCT/colour tile (jd_internal.hpp kTileMaxBlocks)
UNIT = [1] * 64
LONG_BITS = 4 * 8192  # every path of the `decoder` fixture cuts such a stream into several pieces
FAMILIES = ["stair", "edge", "uniform", "pairs", "dense", "six", "ident"]


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------
def _spread(symbols, counts, seed, fixed=None):
    """symbol -> length: `fixed` as given, the other symbols shuffled over counts [(length, n)]."""
    fixed = dict(fixed or {})
    slots = [l for l, n in counts for _ in range(n)]
    for l in fixed.values():
        slots.remove(l)
    rest = [s for s in symbols if s not in fixed]
    assert len(rest) == len(slots), (len(rest), len(slots))
    order = np.random.default_rng(seed).permutation(len(rest))
    out = dict(fixed)
    out.update({rest[int(i)]: l for i, l in zip(order, slots)})
    return out


def _set(y, cb=None, cr=None, ids=((0, 0), (1, 1), (1, 1)), packing="each"):
    """A table set: per component (DC, AC) as jd_coef.canonical lengths or ready (bits, vals)."""
    cb = cb or y
    cr = cr or cb
    tabs = [tuple(t if isinstance(t, tuple) else jd_coef.canonical(t) for t in comp) for comp in (y, cb, cr)]
    return {"tables": tabs, "ids": [tuple(i) for i in ids], "packing": packing}


_STAIR_DC = [(2, 3)] + [(l, 1) for l in range(3, 17)]
_STAIR_AC_Y = [(1, 1)] + [(l, 1) for l in range(3, 9)] + [(9, 4), (10, 8), (11, 16), (12, 30), (13, 40), (14, 50),
                                                           (15, 50), (16, 51)]
_STAIR_AC_C = [(2, 2)] + [(l, 1) for l in range(3, 9)] + [(9, 4), (10, 8), (11, 16), (12, 30), (13, 40), (14, 50),
                                                           (15, 50), (16, 50)]
STAIR_DC_Y = _spread(range(17), _STAIR_DC, 11)
STAIR_DC_C = _spread(range(17), _STAIR_DC, 12)
STAIR_AC_Y = _spread(range(256), _STAIR_AC_Y, 13, {0x00: 4})
STAIR_AC_C = _spread(range(256), _STAIR_AC_C, 14, {0x00: 16})  # EOB behind the longest code

EDGE_DC = {0: 2, 1: 3, 11: 3, 12: 4, 2: 4, 3: 5, 4: 6, 13: 7, 16: 8, 7: 9, 8: 9, 5: 10, 9: 10, 6: 11, 10: 11}
_EDGE_AC = {0x09: 1, 0x08: 2, 0x17: 3, 0x06: 4, 0x05: 5, 0x03: 6, 0x04: 8, 0x31: 9, 0x41: 9, 0x00: 10, 0xF0: 10,
            0x01: 10, 0x15: 10, 0x0A: 10, 0x02: 11, 0x21: 11, 0x0B: 11, 0x0F: 11}
EDGE_AC_A = dict(_EDGE_AC)                                                               # 1 bit: size 9
EDGE_AC_B = {{0x09: 0x0A, 0x0A: 0x09}.get(s, s): l for s, l in _EDGE_AC.items()}          # 1 bit: size 10

_AC255 = [s for s in range(256) if s != 0xFF]


def _uniform(length):
    if length == 16:
        return ({s: 16 if s < 12 else 15 for s in range(17)}, {s: 16 if i < 200 else 15 for i, s in enumerate(_AC255)})
    return ({s: length for s in range(17)}, {s: length for s in _AC255})


PAIR_DC = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 8: 7}
PAIR_T5 = {0x01: 1, 0x00: 2, 0x05: 3, 0x04: 4, 0x03: 5, 0x02: 6, 0xF0: 7, 0x12: 8}
PAIR_T6 = {0x01: 1, 0x06: 2, 0x00: 3, 0xF0: 4, 0x21: 5}
PAIR_T7 = {0x07: 1, 0xF0: 2, 0x00: 3, 0x11: 4, 0x01: 5}
# Complete code (canonical() refuses it; the parsers take it): the only tables in which a pair's
# second symbol has size 8, so the only ones that reach v2 = +-255 and +-128.
PAIR_T8 = ([2] + [0] * 15, [0xF0, 0x08])


def _dense(d):
    a = (d + 1) // 2  # DC size 0 behind a bits, EOB behind d - a: a d-bit block is one region word
    dc = {0: a}
    dc.update({s: 8 + (s > 6) for s in range(1, 12)})
    ac = {0x00: d - a}
    ac.update({s: 9 for s in (0x01, 0x02, 0x03, 0x11, 0x21, 0xF0)})
    ac.update({s: 10 for s in (0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A, 0x31)})
    return dc, ac


DC10 = {0: 2, 1: 2, 2: 3, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 10}  # as an AC table: EOB and run-0 sizes 1..10

IDENT_A = {0x01: 2, 0x02: 2, 0x00: 3, 0x03: 3, 0x11: 4, 0x04: 4, 0xF0: 5, 0x12: 6}
IDENT_B = dict(zip([0x02, 0x01, 0x03, 0x00, 0x04, 0x11, 0x12, 0xF0], IDENT_A.values()))  # A's counts, values permuted
IDENT_C = dict(zip(IDENT_A, [2, 3, 3, 3, 4, 4, 5, 5]))                                 # A's values, other counts


@functools.lru_cache(None)
def table_sets():
    """family -> {set name: table set}."""
    stair = (STAIR_DC_Y, STAIR_AC_Y), (STAIR_DC_C, STAIR_AC_C)
    six_y, six_cb, six_cr = (EDGE_DC, EDGE_AC_A), (DC10, DC10), (STAIR_DC_C, STAIR_AC_C)
    perm = ((3, 2), (0, 3), (1, 0))
    out = {
        "stair": {"stair": _set(*stair)},
        "edge": {"edgeA": _set((EDGE_DC, EDGE_AC_A), (EDGE_DC, EDGE_AC_B), ids=((0, 0), (0, 1), (0, 1))),
                 "edgeB": _set((EDGE_DC, EDGE_AC_B), (EDGE_DC, EDGE_AC_A), ids=((0, 0), (0, 1), (0, 1)))},
        "uniform": {f"uni{l}": _set(_uniform(l), ids=((0, 0), (0, 0), (0, 0))) for l in (10, 11, 16)},
        "pairs": {"p56": _set((PAIR_DC, PAIR_T5), (PAIR_DC, PAIR_T6), ids=((0, 0), (0, 1), (0, 1))),
                  "p65": _set((PAIR_DC, PAIR_T6), (PAIR_DC, PAIR_T5), ids=((0, 0), (0, 1), (0, 1))),
                  "p78": _set((PAIR_DC, PAIR_T7), (PAIR_DC, PAIR_T8), ids=((0, 0), (0, 1), (0, 1))),
                  "p87": _set((PAIR_DC, PAIR_T8), (PAIR_DC, PAIR_T7), ids=((0, 0), (0, 1), (0, 1))),
                  "p66": _set((PAIR_DC, PAIR_T6), ids=((0, 0), (0, 0), (0, 0)))},
        "dense": {f"dense{d}": _set(_dense(d), ids=((0, 0), (0, 0), (0, 0))) for d in range(2, 9)},
        "six": {f"six-{pk}": _set(six_y, six_cb, six_cr, ids=perm, packing=pk)
                for pk in ("each", "one", "each+twice", "one+before_sof", "one+twice+before_sof")},
        "ident": {"identA": _set((PAIR_DC, IDENT_A), ids=((0, 0), (0, 0), (0, 0))),
                  "identB": _set((PAIR_DC, IDENT_B), ids=((0, 0), (0, 0), (0, 0))),
                  "identC": _set((PAIR_DC, IDENT_C), ids=((0, 0), (0, 0), (0, 0))),
                  # the same bytes as a DC table in one file, as an AC table in the next
                  "dc10-dc": _set((DC10, IDENT_A), ids=((0, 0), (0, 0), (0, 0))),
                  "dc10-ac": _set((PAIR_DC, DC10), ids=((0, 0), (0, 0), (0, 0)))},
    }
    out["dc16"] = {"dc16": _set(({0: 1, 1: 2, 2: 3, 15: 15, 16: 16}, PAIR_T5), ids=((0, 0), (0, 0), (0, 0)))}  # dc16_case()
    # five distinct tables: Cr shares Y's DC table (and its id)
    out["six"]["five"] = _set(six_y, six_cb, (EDGE_DC, STAIR_AC_C), ids=((3, 2), (0, 3), (3, 0)))
    return out


def distinct_tables(huff, nc):
    """The LUT slots a frame needs: its distinct (class, counts, values)."""
    return len({(tc, tuple(huff["tables"][c][tc][0]), tuple(huff["tables"][c][tc][1]))
                for c in range(nc) for tc in (0, 1)})


def codes_of(spec):
    """[(symbol, code, length)] in code order (Annex C)."""
    bits, vals = spec
    out, code, k = [], 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out.append((vals[k], code, length))
            code += 1
            k += 1
        code <<= 1
    return out


# ---------------------------------------------------------------------------------------------
# the densest block a table pair allows (the truth behind jd_plan.cpp region_divisor)
# ---------------------------------------------------------------------------------------------
def densest_block(dc, ac, d):
    """max over every symbol sequence that forms one block of d x words - bits, in half-words (so
    2 x that), and the block (DC symbol, [AC symbols]) that attains it.  Words: one record plus half
    a word per entry slot, an escaped value (size >= 10) taking two slots; bits: code + magnitude.
    g[k]: the best from coefficient index k on; a block ends at EOB or when the index passes 63
    (a coefficient that lands past 63 is read and dropped: no slot)."""
    acs = [(sym, length) for sym, _, length in codes_of(ac)]
    g = [(0, None)] * 80
    for k in range(63, 0, -1):
        best = None
        for sym, length in acs:
            if sym == 0:
                cand = -2 * length
            else:
                size, k1 = sym & 15, k + (sym >> 4)
                cand = -2 * (length + size)
                if k1 < 64:
                    cand += d * (0 if size == 0 else 1 if size <= 9 else 2) + (g[k1 + 1][0] if k1 + 1 < 64 else 0)
            if best is None or cand > best[0]:
                best = (cand, sym)
        g[k] = best
    dsym, dbits = min(((sym, length + sym) for sym, _, length in codes_of(dc)), key=lambda t: t[1])
    block, k = [], 1
    while k < 64:
        sym = g[k][1]
        block.append(sym)
        if sym == 0:
            break
        k += (sym >> 4) + 1
    return 2 * d - 2 * dbits + g[1][0], (dsym, block)


def true_divisor(huff, nc):
    """The largest d in 2..8 such that no block of any component fills more than one region word per
    d walk bits.  (A block is decoded with one component's DC and AC table, in or out of step.)"""
    d = 8
    while d > 2 and any(densest_block(*huff["tables"][c], d)[0] > 0 for c in range(nc)):
        d -= 1
    assert all(densest_block(*huff["tables"][c], 2)[0] <= 0 for c in range(nc))  # every item takes >= 2 bits
    return d


# ---------------------------------------------------------------------------------------------
# random coefficients within a table set
# ---------------------------------------------------------------------------------------------
def _value(rng, size):
    """A value of `size` magnitude bits, the four extremes of the size more often than the rest."""
    if size == 0:
        return 0
    lo, hi = 1 << (size - 1), (1 << size) - 1
    mag = int(rng.choice([lo, hi])) if rng.random() < 0.3 else int(rng.integers(lo, hi + 1))
    return mag if rng.random() < 0.5 else -mag


def _ac_options(ac_syms):
    """size -> runs r (0..63) a coefficient of that size can follow: symbol (r mod 16, size), and
    ZRL when r > 15."""
    zrl = 0xF0 in ac_syms
    opts = {}
    for sym in ac_syms:
        if sym & 15:
            opts.setdefault(sym & 15, []).extend((sym >> 4) + 16 * j for j in range(4 if zrl else 1))
    return opts


def _random_block(rng, zz, opts, has_eob, full):
    """Fills zz[1:]: the size drawn first (uniform over the sizes the table carries), then the run
    among those the table codes for it.  full (or a table without EOB): the block reaches position
    63, when the table allows it."""
    full = full or not has_eob
    k, n = 1, int(rng.integers(0, 24))
    sizes = sorted(opts)
    for i in range(200):
        if k > 63 or (not full and i >= n):
            break
        size = sizes[int(rng.integers(0, len(sizes)))]
        runs = [r for r in opts[size] if k + r <= 63]
        if full and i >= n:  # finish: land on 63 if a symbol does, else take the shortest step
            last = [(s, 63 - k) for s in sizes if 63 - k in opts[s]]
            if last:
                size, runs = last[int(rng.integers(0, len(last)))][0], [63 - k]
            else:
                steps = [(min(r for r in opts[s] if k + r <= 63), s) for s in sizes if any(k + r <= 63 for r in opts[s])]
                if not steps:
                    break
                r, size = min(steps)
                runs = [r]
        if not runs:
            continue
        k += runs[int(rng.integers(0, len(runs)))]
        zz[k] = _value(rng, size)
        k += 1
    assert has_eob or zz[63] != 0


def random_coefs(seed, width, height, factors, huff, restart=0, full_p=0.15, dense=None):
    """Coefficient arrays for one image.  DC differences: size uniform over the DC table's symbols,
    the sign mostly towards zero (the absolute DC stays within a few times 65535).  dense: (DC
    symbol, AC symbols) of a block that every other MCU row repeats (unit magnitudes)."""
    rng = np.random.default_rng(seed)
    nc = len(factors)
    coefs = [np.zeros(s, np.int32) for s in jd_coef.coef_shapes(width, height, factors)]
    eff = [(1, 1)] if nc == 1 else factors
    bpm = sum(h * v for h, v in eff)
    _, _, mcux, _ = jd_coef.grid(width, height, factors)
    syms = [([s for s, _, _ in codes_of(huff["tables"][c][0])], [s for s, _, _ in codes_of(huff["tables"][c][1])])
            for c in range(nc)]
    opts = [_ac_options(a) for _, a in syms]
    pred = [0] * nc
    for n, (c, row, col) in enumerate(jd_coef.scan_blocks(width, height, factors)):
        if restart and n % (restart * bpm) == 0:
            pred = [0] * nc
        zz = coefs[c][row, col]
        if dense is not None and (n // (bpm * mcux)) % 2 == 0:
            dsym, block = dense
            diff = 0 if dsym == 0 else 1 << (dsym - 1)
            zz[:] = jd_coef.coefs_of_symbols((dsym, diff), [(s, (1 << ((s & 15) - 1)) if s & 15 else 0) for s in block],
                                             pred[c])
        else:
            size = syms[c][0][int(rng.integers(0, len(syms[c][0])))]
            diff = abs(_value(rng, size))
            if (pred[c] > 0) == (rng.random() < 0.7):
                diff = -diff
            zz[0] = pred[c] + diff
            _random_block(rng, zz, opts[c], 0 in syms[c][1], rng.random() < full_p)
        pred[c] = int(zz[0])
    return coefs


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def _finish(family, tset, tag, layout, width, height, huff, restart, coefs, symbols=None):
    f = LAYOUTS[layout]
    info = {}
    data = jd_coef.build(width, height, f, None if symbols else coefs, [UNIT, UNIT], restart=restart, huff=huff,
                         symbols=symbols, info=info)
    return SimpleNamespace(id=f"{tset}-{layout}-{tag}", family=family, tset=tset, layout=layout, width=width,
                           height=height, factors=f, coefs=coefs, symbols=symbols, huff=huff, restart=restart,
                           data=data, bits=info["bits"], long=tag.startswith("long"),
                           ref=jd_coef.reference(width, height, f, coefs, [UNIT, UNIT]))


def _small(family, tset, layout, seed, **kw):
    huff = table_sets()[family][tset]
    f = LAYOUTS[layout]
    return _finish(family, tset, "5x3", layout, 5, 3, huff, 0, random_coefs(seed, 5, 3, f, huff, **kw))


def _odd_restart(layout):
    bpm = sum(h * v for h, v in LAYOUTS[layout])
    return next(r for r in range(2, 64) if (TILE_BLOCKS // bpm) % r)  # no divisor of the tile's MCU count


def _long(family, tset, layout, restart, seed, **kw):
    """More than one IDCT tile wide, odd width and height, as many MCU rows as LONG_BITS takes."""
    huff = table_sets()[family][tset]
    f = LAYOUTS[layout]
    hmax, vmax, bpm = max(h for h, _ in f), max(v for _, v in f), sum(h * v for h, v in f)
    width = 8 * hmax * (TILE_BLOCKS // bpm + 1) - 3
    rows = 2
    while True:
        height = 8 * vmax * rows - 1
        case = _finish(family, tset, f"long-rst{restart}", layout, width, height, huff, restart,
                       random_coefs(seed, width, height, f, huff, restart, **kw))
        if case.bits >= LONG_BITS:
            return case
        rows = max(rows + 1, int(rows * LONG_BITS / case.bits) + 1)


def _trio(family, tsets, seed, **kw):
    """A 5 x 3 image and long images over the three layouts and the three restart settings, the
    family's table sets taken in turn."""
    out = [_small(family, tsets[0], "4:4:4", seed, **kw)]
    for i, (layout, rst) in enumerate((("gray", 0), ("4:4:4", 1), ("4:2:0", None))):
        for j, ts in enumerate(tsets if len(tsets) <= 2 else [tsets[i % len(tsets)]]):
            out.append(_long(family, ts, layout, _odd_restart(layout) if rst is None else rst, seed + 10 * i + j + 1, **kw))
    return out


def _pattern_case(family, tset, tag, patterns, seed):
    """Symbol-level 4:4:4 image: block n carries patterns[n % len] as its AC symbols (values drawn for
    the sizes), random DC differences; its coefficients are what coefs_of_symbols() states."""
    huff = table_sets()[family][tset]
    rng = np.random.default_rng(seed)
    width, height, f = 8 * 7 - 3, 8 * 3 - 1, LAYOUTS["4:4:4"]
    symbols = []
    for n, (c, _, _) in enumerate(jd_coef.scan_blocks(width, height, f)):
        dsyms = [s for s, _, _ in codes_of(huff["tables"][c][0])]
        diff = _value(rng, dsyms[int(rng.integers(0, len(dsyms)))])
        symbols.append(((int(abs(diff)).bit_length(), diff),
                        [(s, _value(rng, s & 15)) for s in patterns[(n // 3 + c) % len(patterns)]]))
    coefs = jd_coef.coefs_of_scan(width, height, f, symbols)
    return _finish(family, tset, tag, "4:4:4", width, height, huff, 0, coefs, symbols)


# stair (all 256 AC symbols): a run past 63 whose value is dropped, ZRL landing on 63 and going
# past it, size-0 symbols with runs 1..14 (alone, and between coefficients)
_STAIR_PATTERNS = [
    [0x01] * 59 + [0x53],                                  # k = 60: 60 + 5 > 63, three bits read and dropped
    [0x02] * 47 + [0xF0],                                  # k = 48: ZRL's zero lands on 63
    [0x01] * 49 + [0xF0],                                  # k = 50: ZRL runs past 63
    [0x10, 0x20, 0x30, 0x40, 0x50, 0x60, 0x70, 0x80, 0x90, 0xA0],
    [0xB0, 0xC0, 0xD0, 0xE0, 0x00],
    [0x30, 0x02, 0x10, 0x7C, 0xE0, 0x11, 0x00],
    [0xF0, 0xF0, 0xF0, 0xFA],                              # k = 49: 49 + 15 > 63, ten bits dropped
]
# pairs (T6 in every component): the second symbol of a pair runs past 63; the first one does
_PAIR_PATTERNS = [
    [0x01] * 61 + [0x21],                                  # 0x01 lands on 61, its partner 0x21 (run 2) is dropped
    [0xF0, 0xF0, 0xF0] + [0x01] * 13 + [0x21],             # k = 62: the first symbol of the entry is dropped
    [0x01] * 61 + [0x06, 0x01],                            # ends on 63 with the pair 0x06, 0x01
    [0x06, 0x00],
]


@functools.lru_cache(None)
def family_cases(family):
    ts = list(table_sets()[family])
    if family == "stair":
        return _trio(family, ts, 100) + [_pattern_case(family, "stair", "symbols", _STAIR_PATTERNS, 190)]
    if family == "edge":
        return _trio(family, ts, 200)
    if family == "uniform":
        return _trio(family, ts, 300)
    if family == "pairs":
        out = _trio(family, ts[:2], 400, full_p=0.4) + _trio(family, ts[2:4], 450, full_p=0.4)
        return out + [_pattern_case(family, "p66", "symbols", _PAIR_PATTERNS, 490)]
    if family == "dense":
        # d = 2: 16384 two-bit blocks (a 1-bit DC code for size 0, a 1-bit EOB): LONG_BITS exactly
        huff = table_sets()[family]["dense2"]
        block = densest_block(*huff["tables"][0], 2)[1]
        assert block == (0, [0])
        out = [_small(family, "dense2", "gray", 500, dense=block)]
        for rst in (0, 1, 7):
            coefs = [np.zeros(s, np.int32) for s in jd_coef.coef_shapes(1024, 1024, LAYOUTS["gray"])]
            out.append(_finish(family, "dense2", f"long-rst{rst}", "gray", 1024, 1024, huff, rst, coefs))
        for i, d in enumerate(range(3, 9)):  # the densest block in every other MCU row, random ones between
            layout = ("4:4:4", "4:2:0", "gray")[i % 3]
            huff = table_sets()[family][f"dense{d}"]
            out.append(_long(family, f"dense{d}", layout, (0, 1, _odd_restart(layout))[(i // 3 + i) % 3], 510 + d,
                             dense=densest_block(*huff["tables"][0], d)[1]))
        return out
    if family == "six":
        out = [_small(family, t, "4:4:4", 600 + i) for i, t in enumerate(ts)]
        out += [_long(family, "six-each", "4:2:0", 0, 650), _long(family, "six-one+twice+before_sof", "4:4:4", 1, 651),
                _long(family, "five", "4:2:0", _odd_restart("4:2:0"), 652), _long(family, "five", "gray", 0, 653)]
        return out
    if family == "ident":
        return [_small(family, t, "4:4:4", 700 + i) for i, t in enumerate(ts)]
    raise KeyError(family)


@functools.lru_cache(None)
def dc16_case():
    """The one symbol the device entry format cannot hold (jd_internal.hpp lut_entry: l + size > 31):
    a DC size 16 behind a 16-bit code.  No family table has it (tests/test_huff_ref.py asserts so);
    this gray image of four blocks is made of it."""
    coefs = [np.zeros(s, np.int32) for s in jd_coef.coef_shapes(16, 16, LAYOUTS["gray"])]
    coefs[0][..., 0] = [[40000, -25535], [-25534, 40001]]  # differences +40000, -65535, +1, +65535
    coefs[0][..., 1] = 3
    return _finish("dc16", "dc16", "4blocks", "gray", 16, 16, table_sets()["dc16"]["dc16"], 0, coefs)


def all_cases():
    return [c for f in FAMILIES for c in family_cases(f)]


@functools.lru_cache(None)
def oracle_outputs():
    """id -> (status, pixels) of jdoracle.decode for every case, computed once per process."""
    import jdoracle

    return {c.id: jdoracle.decode(c.data) for c in all_cases()}
