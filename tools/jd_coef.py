"""Coefficient-level baseline JPEG builder and a plain reference decode of the same coefficients.

build() writes a valid baseline stream from quantised coefficients chosen by the caller, for any
sampling layout the parser accepts (factors 1, 2, 4; at most 10 blocks per MCU), 8- or 16-bit
quantisation tables and any restart interval; with the Annex K.3 Huffman tables below, or with
tables given per component (huff=: any DHT ids and packing, DC sizes to 16, AC sizes to 15;
canonical() makes a table from code lengths), from coefficients or, for the sequences no
coefficients produce, from the symbols themselves (symbols=, coefs_of_symbols()).  reference() computes the RGB of the same
coefficients directly: dequantise, IDCT per block (jdoracle.idct, pinned to the reference decoder
by the ground-truth fixtures), planes, replicate upsampling, colour in float64 / float32 as the
reference rounds.  It reads no bitstream and shares no layout or colour code with
oracle/jdoracle.c or the kernels.  Test infrastructure only (pure Python + numpy).
"""
from __future__ import annotations

import os
import sys

import numpy as np

# Annex K.3 Huffman tables.  The DC table is the luminance one extended by symbol 12 on the free
# 10-bit code, so absolute DCs of +-2047 (differences up to +-4094) are expressible.
DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
DC_VALS = list(range(13))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]

# natural (row-major) index of zig-zag position k
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63]


def _codes(bits, vals):
    """symbol -> (code, length), Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def grid(width, height, factors):
    """(hmax, vmax, mcux, mcuy) of a frame; a single component is one block per MCU."""
    if len(factors) == 1:
        factors = [(1, 1)]
    hmax = max(h for h, _ in factors)
    vmax = max(v for _, v in factors)
    return hmax, vmax, -(-width // (8 * hmax)), -(-height // (8 * vmax))


def coef_shapes(width, height, factors):
    """[block_rows, block_cols, 64] of every component's coefficient array (padded MCU grid)."""
    _, _, mcux, mcuy = grid(width, height, factors)
    if len(factors) == 1:
        factors = [(1, 1)]
    return [(mcuy * v, mcux * h, 64) for h, v in factors]


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.total = 0  # bits put, padding included

    def put(self, value, length):
        self.total += length
        self.acc = (self.acc << length) | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)  # stuffing
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)  # 1-bits to the byte boundary


def _magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


def canonical(lengths):
    """(bits[16], vals) of the canonical code with the given symbol -> code length (1..16); symbols
    of one length keep the mapping's order.  Rejects what a DHT segment cannot carry or Annex C
    forbids: an over-subscribed set, one that uses the all-ones code of its longest length (a
    complete set does), more than 255 codes of one length (a DHT count is one byte)."""
    bits = [0] * 16
    for sym, length in lengths.items():
        if not (0 <= sym <= 255 and 1 <= length <= 16):
            raise ValueError(f"symbol {sym} / length {length} out of range")
        bits[length - 1] += 1
    if not lengths:
        raise ValueError("empty code")
    if max(bits) > 255:
        raise ValueError("more than 255 codes of one length")
    kraft = sum(n << (16 - l) for l, n in enumerate(bits, start=1))
    if kraft > 1 << 16:
        raise ValueError("over-subscribed code lengths")
    if kraft == 1 << 16:
        raise ValueError("the all-ones code of the longest length is in use")
    vals = [sym for sym, _ in sorted(lengths.items(), key=lambda kv: kv[1])]  # stable: mapping order
    return bits, vals


def scan_blocks(width, height, factors):
    """(component, block row, block column) of every block in scan order (MCU by MCU)."""
    _, _, mcux, mcuy = grid(width, height, factors)
    eff = [(1, 1)] if len(factors) == 1 else list(factors)
    return [(c, my * v + by, mx * h + bx) for my in range(mcuy) for mx in range(mcux)
            for c, (h, v) in enumerate(eff) for by in range(v) for bx in range(h)]


def symbols_of_block(zz, pred):
    """Coefficients -> symbols: ((size, diff), [(run/size byte, value), ...]) of one block, as an
    encoder writes them (ZRL for runs beyond 15, EOB unless position 63 is non-zero)."""
    diff = int(zz[0]) - pred
    acs = []
    run = 0
    nz = np.flatnonzero(zz[1:])
    last = int(nz[-1]) + 1 if nz.size else 0
    for k in range(1, last + 1):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            acs.append((0xF0, 0))
            run -= 16
        if abs(v) > 32767:
            raise ValueError(f"AC coefficient {v} beyond size 15")
        acs.append(((run << 4) | int(abs(v)).bit_length(), v))
        run = 0
    if last < 63:
        acs.append((0x00, 0))
    return (int(abs(diff)).bit_length(), diff), acs


def coefs_of_symbols(dc, acs, pred):
    """Symbols -> the 64 coefficients (zig-zag, absolute DC) the reference decodes from them
    (parser.cpp:114-134): k += run; read the magnitude; store it only if k < 64; k++; the block
    ends at EOB or at k >= 64.  Symbols after the block's end are an error of the caller."""
    zz = np.zeros(64, np.int32)
    zz[0] = pred + dc[1]
    k = 1
    for i, (rs, value) in enumerate(acs):
        if k >= 64:
            raise ValueError("symbols after the block's end")
        if rs == 0:
            if i != len(acs) - 1:
                raise ValueError("symbols after EOB")
            return zz
        k += rs >> 4
        if k < 64:
            zz[k] = value if rs & 15 else 0
            k += 1
    if k < 64:
        raise ValueError("block neither ends with EOB nor reaches position 63")
    return zz


def coefs_of_scan(width, height, factors, symbols, restart=0):
    """The coefficient arrays (coef_shapes) that a scan's symbols decode to, block by block through
    coefs_of_symbols(), the DC prediction reset at every restart interval."""
    nc = len(factors)
    coefs = [np.zeros(s, np.int32) for s in coef_shapes(width, height, factors)]
    bpm = sum(h * v for h, v in ([(1, 1)] if nc == 1 else factors))
    pred = [0] * nc
    for n, (c, row, col) in enumerate(scan_blocks(width, height, factors)):
        if restart and n % (restart * bpm) == 0:
            pred = [0] * nc
        coefs[c][row, col] = coefs_of_symbols(*symbols[n], pred[c])
        pred[c] = int(coefs[c][row, col, 0])
    return coefs


def _put_symbols(bw, dc, acs, dc_codes, ac_codes):
    """Symbols -> bits.  The size limits are the tables': a symbol they lack is an error."""
    size, diff = dc
    if size != int(abs(diff)).bit_length() or size > 16:
        raise ValueError(f"DC difference {diff} is not of size {size}")
    if size not in dc_codes:
        raise ValueError(f"DC difference {diff} (size {size}) beyond the DC table")
    bw.put(*dc_codes[size])
    if size:
        bw.put(_magnitude(diff)[1], size)
    for rs, value in acs:
        if rs not in ac_codes:
            raise ValueError(f"AC symbol {rs:#04x} (value {value}) beyond the AC table")
        bw.put(*ac_codes[rs])
        size = rs & 15
        if size:
            if size != int(abs(value)).bit_length():
                raise ValueError(f"AC value {value} is not of size {size}")
            bw.put(_magnitude(value)[1], size)


_ANNEX_K = {"tables": [((DC_BITS, DC_VALS), (AC_LUMA_BITS, AC_LUMA_VALS))] +
                      [((DC_BITS, DC_VALS), (AC_CHROMA_BITS, AC_CHROMA_VALS))] * 2,
            "ids": [(0, 0), (0, 1), (0, 1)], "packing": "each"}


def _dht_segments(huff, nc):
    """The DHT segments of a table set (see build()): (before SOF, after SOF)."""
    flags = set(huff.get("packing", "each").split("+"))
    assert flags <= {"each", "one", "twice", "before_sof"} and not {"each", "one"} <= flags
    defs = {}  # (class, id) -> (bits, vals), in order of first use
    for c in range(nc):
        for tc in (0, 1):
            spec, th = huff["tables"][c][tc], huff["ids"][c][tc]
            bits, vals = [int(x) for x in spec[0]], [int(x) for x in spec[1]]
            assert 0 <= th <= 3 and len(bits) == 16 and sum(bits) == len(vals) and max(bits) <= 255
            assert defs.setdefault((tc, th), (bits, vals)) == (bits, vals), "one id, two tables"
    body = [bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals) for (tc, th), (bits, vals) in defs.items()]
    if "twice" in flags:  # every id first defined with another table (the later definition wins)
        decoy = {0: (DC_BITS, DC_VALS), 1: (AC_LUMA_BITS, AC_LUMA_VALS)}
        body = [bytes([(tc << 4) | th]) + bytes(decoy[tc][0]) + bytes(decoy[tc][1]) for tc, th in defs] + body
    segs = [_segment(0xC4, b"".join(body))] if "one" in flags else [_segment(0xC4, b) for b in body]
    return (b"".join(segs), b"") if "before_sof" in flags else (b"", b"".join(segs))


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def build(width, height, factors, coefs, qtabs, tq=None, restart=0, comp_ids=(1, 2, 3), huff=None, symbols=None,
          info=None):
    """Baseline JPEG bytes.  factors: (h, v) per component; coefs[c]: int [block_rows, block_cols,
    64], zig-zag order, absolute DC, before dequantisation, on the padded MCU grid (coef_shapes);
    qtabs: 64-entry tables in zig-zag order (an entry above 255 makes the table 16-bit); tq: table
    index per component (default: 0 for the first, the last table for the others); restart: MCUs
    per restart interval (0: none).
    huff: None for the Annex K set above, else {"tables": per component ((bits, vals) DC, (bits,
    vals) AC), "ids": per component (Td, Ta), the DHT ids 0..3 the tables are written under and the
    SOS selects, "packing": "each" (one DHT segment per table) or "one" (all in one segment),
    optionally with "+twice" (every id defined first with another table) and "+before_sof"}.
    symbols: instead of coefs (None), per block in scan order ((size, diff), [(run/size byte,
    value), ...]), written as given (coefs_of_symbols() says what they decode to).
    info: a dict that receives "bits", the entropy-coded bits written (padding included)."""
    nc = len(factors)
    assert nc in (1, 3) and (symbols is None) != (coefs is None)
    nblocks = len(scan_blocks(width, height, factors))
    if symbols is None:
        assert len(coefs) == nc
    else:
        assert len(symbols) == nblocks
    if tq is None:
        tq = [0] + [len(qtabs) - 1] * (nc - 1)
    hmax, vmax, mcux, mcuy = grid(width, height, factors)
    eff = [(1, 1)] if nc == 1 else list(factors)  # a single-component scan is not interleaved
    for c, shape in enumerate(coef_shapes(width, height, factors) if symbols is None else []):
        assert tuple(coefs[c].shape) == shape, (c, coefs[c].shape, shape)
    out = bytearray(b"\xff\xd8")
    for t, q in enumerate(qtabs):
        q = [int(x) for x in q]
        assert len(q) == 64 and all(1 <= x <= 65535 for x in q)
        if max(q) > 255:
            out += _segment(0xDB, bytes([0x10 | t]) + b"".join(x.to_bytes(2, "big") for x in q))
        else:
            out += _segment(0xDB, bytes([t]) + bytes(q))
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        sof += bytes([comp_ids[c], (factors[c][0] << 4) | factors[c][1], tq[c]])
    if huff is None:
        huff = _ANNEX_K
    dht_before, dht_after = _dht_segments(huff, nc)
    out += dht_before + _segment(0xC0, sof) + dht_after
    codes = [(_codes(*huff["tables"][c][0]), _codes(*huff["tables"][c][1])) for c in range(nc)]
    if restart:
        out += _segment(0xDD, int(restart).to_bytes(2, "big"))
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([comp_ids[c], (huff["ids"][c][0] << 4) | huff["ids"][c][1]])
    out += _segment(0xDA, sos + bytes([0, 63, 0]))
    bw = _Bits()
    pred = [0] * nc
    rst = 0
    bpm = sum(h * v for h, v in eff)
    for n, (c, row, col) in enumerate(scan_blocks(width, height, factors)):
        if restart and n and n % (restart * bpm) == 0:
            bw.flush()
            bw.out += bytes([0xFF, 0xD0 + (rst & 7)])
            rst += 1
            pred = [0] * nc
        if symbols is None:
            dc, acs = symbols_of_block(coefs[c][row, col], pred[c])
        else:
            dc, acs = symbols[n]
        _put_symbols(bw, dc, acs, *codes[c])
        pred[c] += dc[1]
    bw.flush()
    if info is not None:
        info["bits"] = bw.total
    out += bw.out
    out += b"\xff\xd9"
    return bytes(out)


def dequantised(coefs, qtabs, tq=None):
    """Per component: coefficient x step in int32 (wrapping, as the decoders' int arithmetic)."""
    nc = len(coefs)
    if tq is None:
        tq = [0] + [len(qtabs) - 1] * (nc - 1)
    out = []
    for c in range(nc):
        q = np.asarray(qtabs[tq[c]], dtype=np.int64)
        out.append((np.asarray(coefs[c], dtype=np.int64) * q).astype(np.int32))
    return out


def planes(width, height, factors, coefs, qtabs, tq=None):
    """IDCT output of every component as an int32 plane on the padded MCU grid."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "oracle"))
    import jdoracle

    out = []
    for deq in dequantised(coefs, qtabs, tq):
        rows, cols, _ = deq.shape
        px = jdoracle.idct(deq.reshape(-1, 64)).reshape(rows, cols, 8, 8)
        out.append(px.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8))
    return out


def upsampled(width, height, factors, pl):
    """(Y, Cb, Cr) int32 [H, W]: the sample of component c for pixel (x, y) is plane c at
    [y * v // vmax, x * h // hmax]; a single component has Cb = Cr = 0."""
    hmax, vmax, _, _ = grid(width, height, factors)
    eff = [(1, 1)] if len(factors) == 1 else factors
    ys = np.arange(height)[:, None]
    xs = np.arange(width)[None, :]
    full = [pl[c][ys * v // vmax, xs * h // hmax] for c, (h, v) in enumerate(eff)]
    while len(full) < 3:
        full.append(np.zeros((height, width), np.int32))
    return full


def colour(y, cb, cr):
    """The reference's colour formula, float64 products stored to float32 (utils/color.cpp)."""
    yd = y.astype(np.float64)
    r = (cr * (2 - 2 * 0.299) + yd).astype(np.float32)
    b = (cb * (2 - 2 * 0.114) + yd).astype(np.float32)
    g = ((yd - 0.114 * b.astype(np.float64) - 0.299 * r.astype(np.float64)) / 0.587).astype(np.float32)
    return np.stack([np.clip((r + np.float32(128)).astype(np.int32), 0, 255),
                     np.clip((g + np.float32(128)).astype(np.int32), 0, 255),
                     np.clip((b + np.float32(128)).astype(np.int32), 0, 255)], -1).astype(np.uint8)


def reference(width, height, factors, coefs, qtabs, tq=None):
    """uint8 [H, W, 3] of the coefficients build() would encode."""
    y, cb, cr = upsampled(width, height, factors, planes(width, height, factors, coefs, qtabs, tq))
    return colour(y, cb, cr)


def exact_class(cb, cr):
    """True where the chroma pair takes the kernels' double-precision G path: N = 202008 cb +
    419198 cr is non-zero and within 64 of a multiple of 587000 (jd_kernels.hip chroma_terms)."""
    n = 202008 * np.asarray(cb, dtype=np.int64) + 419198 * np.asarray(cr, dtype=np.int64)
    rem = np.mod(n, 587000)
    return (n != 0) & ((rem < 64) | (rem > 587000 - 64))
