"""CPU: the Huffman table space (tests/huff_cases.py) against the coefficient reference, the
coverage audits of those inputs, build_lut entry by entry, and region_divisor against the densest
block the tables allow.

Reference: tools/jd_coef.py reference() of the coefficients a case chose (it never sees a table or
a bit).  Witnesses that must agree with it before anything runs on the GPU: jdoracle.decode,
jdoracle.decode_fast, jdoracle.decode_coefs and tools/jd_trace.py's symbol decoder.  The table
format is checked against lut_model() below, a restatement of the layout documented in
jd_internal.hpp that shares no code with jd_parse.cpp build_lut; the audits walk every stream
with that model and count which kinds of index entry the walk meets.  The same cases run on the
GPU in tests/test_gpu_huff.py.
"""
import collections
import functools
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import huff_cases as hc
import jdoracle
import layout_cases as lc

import jd_coef  # noqa: E402  (tools/ is on the path once huff_cases is imported)
import jd_trace  # noqa: E402

PKG = os.path.join(hc.ROOT, "gpu-jpeg-decoder_amd")
LUT_BITS = 10  # jd_internal.hpp kLutBits


# ---------------------------------------------------------------------------------------------
# the builder
# ---------------------------------------------------------------------------------------------
def test_layout_streams_did_not_move():
    """Every tests/layout_cases.py stream is byte for byte what the builder wrote before it took
    tables as an input (digest over id, length and bytes of all 111, taken from that version)."""
    h = hashlib.sha256()
    for c in lc.all_cases():
        h.update(c.id.encode())
        h.update(len(c.data).to_bytes(4, "little"))
        h.update(c.data)
    assert len(lc.all_cases()) == 111
    assert h.hexdigest() == "b89e400444c3b9270e1f261248750f578e5781b7527e33df42293ef63ae658e6"


def test_canonical_rejects_what_a_dht_cannot_carry():
    bits, vals = jd_coef.canonical({5: 3, 7: 1, 9: 3, 1: 4})
    assert bits == [1, 0, 2, 1] + [0] * 12 and vals == [7, 5, 9, 1]  # one length: the mapping's order
    with pytest.raises(ValueError, match="over-subscribed"):
        jd_coef.canonical({0: 1, 1: 1, 2: 2})
    with pytest.raises(ValueError, match="all-ones"):
        jd_coef.canonical({0: 1, 1: 2, 2: 2})
    with pytest.raises(ValueError, match="all-ones"):
        jd_coef.canonical({0: 1, 1: 1})
    with pytest.raises(ValueError, match="255"):
        jd_coef.canonical({s: 16 for s in range(256)})
    assert jd_coef.canonical({s: 16 if s else 15 for s in range(256)})[0][14:] == [1, 255]
    with pytest.raises(ValueError):
        jd_coef.canonical({0: 17})


def test_builder_takes_its_limits_from_the_tables():
    f, q = hc.LAYOUTS["gray"], [hc.UNIT]
    zz = np.zeros((1, 1, 64), np.int32)
    pairs = hc.table_sets()["pairs"]["p56"]
    zz[0, 0, 0] = 255  # size 8: in PAIR_DC
    jd_coef.build(8, 8, f, [zz], q, huff=pairs)
    zz[0, 0, 0] = 64   # size 7: not in it
    with pytest.raises(ValueError, match="DC table"):
        jd_coef.build(8, 8, f, [zz], q, huff=pairs)
    zz[0, 0, 0], zz[0, 0, 5] = 0, 64  # AC size 7 after a run of 4: not in PAIR_T5
    with pytest.raises(ValueError, match="AC table"):
        jd_coef.build(8, 8, f, [zz], q, huff=pairs)
    stair = hc.table_sets()["stair"]["stair"]
    zz[0, 0, 0], zz[0, 0, 5] = -65535, -32767  # DC size 16, AC size 15
    st, got = jdoracle.decode_coefs(jd_coef.build(8, 8, f, [zz], q, huff=stair))
    assert st == 0 and np.array_equal(got[0], zz[0, 0])
    zz[0, 0, 0] = 65536
    with pytest.raises(ValueError):
        jd_coef.build(8, 8, f, [zz], q, huff=stair)
    zz[0, 0, 0], zz[0, 0, 5] = 0, 32768
    with pytest.raises(ValueError):
        jd_coef.build(8, 8, f, [zz], q, huff=stair)


def test_coefs_of_symbols_states_the_rule():
    """parser.cpp:114-134 on the sequences no coefficients produce."""
    c = jd_coef.coefs_of_symbols
    zz = c((3, -5), [(0x01, 1)] * 59 + [(0x53, 7)], 10)  # k = 60 + 5: read and dropped
    assert zz[0] == 5 and zz[1:60].tolist() == [1] * 59 and not zz[60:].any()
    assert not c((0, 0), [(0x02, 2)] * 47 + [(0xF0, 0)], 0)[48:].any()      # ZRL lands on 63
    assert not c((0, 0), [(0x01, 1)] * 49 + [(0xF0, 0)], 0)[50:].any()      # ZRL runs past it
    zz = c((0, 0), [(0x30, 0), (0x02, 3), (0x00, 0)], 0)                   # a size-0 symbol takes run + 1 places
    assert zz[5] == 3 and np.count_nonzero(zz) == 1
    with pytest.raises(ValueError):
        c((0, 0), [(0x01, 1)], 0)                                          # neither EOB nor position 63
    with pytest.raises(ValueError):
        c((0, 0), [(0x01, 1)] * 63 + [(0x00, 0)], 0)                       # a symbol after the block's end


def test_family_shapes():
    """Per family: gray, 4:4:4 and 4:2:0, a 5 x 3 image, long images of at least 4 x 8192
    entropy-coded bits with restart intervals 0, 1 and a non-divisor of the tile's MCU count."""
    for fam in hc.FAMILIES[:-1]:
        cs = hc.family_cases(fam)
        assert any((c.width, c.height) == (5, 3) for c in cs), fam
        longs = [c for c in cs if c.long]
        assert all(c.bits >= hc.LONG_BITS for c in longs), [(c.id, c.bits) for c in longs]
        if fam != "dense":
            assert all(c.width * c.height < 32768 for c in cs), fam  # under a pixel per bit
        assert {c.layout for c in cs} == set(hc.LAYOUTS), fam
        rst = {c.restart for c in longs}
        assert {0, 1} <= rst and any(r > 1 and (hc.TILE_BLOCKS // sum(h * v for h, v in c.factors)) % r
                                     for c in longs for r in [c.restart]), fam
    ids = [c.id for c in hc.all_cases()]
    assert len(ids) == len(set(ids))
    d2 = [c for c in hc.family_cases("dense") if c.tset == "dense2" and c.long]
    assert [(c.width, c.height, c.restart) for c in d2] == [(1024, 1024, r) for r in (0, 1, 7)]
    assert d2[0].bits == hc.LONG_BITS  # 16384 blocks of 2 bits
    # what the families are made of
    stair = hc.table_sets()["stair"]["stair"]["tables"]
    assert sorted(stair[0][0][1]) == list(range(17)) and sorted(stair[0][1][1]) == list(range(256))
    assert sorted(stair[1][1][1]) == list(range(256))
    assert all(n > 0 for n in stair[0][1][0][2:]) and stair[0][1][0][0] == 1 and all(n > 0 for n in stair[1][1][0][1:])
    for l, t in ((10, "uni10"), (11, "uni11")):
        for spec in hc.table_sets()["uniform"][t]["tables"][0]:
            assert [i + 1 for i, n in enumerate(spec[0]) if n] == [l]
    assert all([i + 1 for i, n in enumerate(spec[0]) if n] == [15, 16] for spec in hc.table_sets()["uniform"]["uni16"]["tables"][0])
    six = hc.table_sets()["six"]["six-each"]
    assert six["tables"][1][0] == six["tables"][1][1]  # the AC table's bytes are the DC table's
    assert sorted(i for c in six["ids"] for i in c[:1]) == [0, 1, 3] and sorted(c[1] for c in six["ids"]) == [0, 2, 3]
    a, b, c = (hc.table_sets()["ident"][t]["tables"][0][1] for t in ("identA", "identB", "identC"))
    assert a[0] == b[0] and a[1] != b[1] and sorted(a[1]) == sorted(b[1])  # equal counts, permuted values
    assert a[1] == c[1] and a[0] != c[0]                                   # equal values, other counts


def test_dc_size16_behind_a_16_bit_code():
    """The device entry format cannot hold this symbol (tests/test_gpu_huff.py pins what the GPU
    reports); no family table has it, and the oracle decodes hc.dc16_case() to the reference."""
    for fam in hc.FAMILIES:
        for ts in hc.table_sets()[fam].values():
            for comp in ts["tables"]:
                assert not any(sym == 16 and length == 16 for sym, _, length in hc.codes_of(comp[0]))
    c = hc.dc16_case()
    assert (16, 16) in [(sym, length) for sym, _, length in hc.codes_of(c.huff["tables"][0][0])]
    for got in (jdoracle.decode(c.data), jdoracle.decode_fast(c.data)):
        assert got[0] == 0 and np.array_equal(got[1], c.ref)
    assert np.array_equal(jdoracle.decode_coefs(c.data)[1], _scan_coefs(c))
    assert np.array_equal(_trace_coefs(c.data), _scan_coefs(c))


def test_slot_counts():
    """Table sets of 2, 3, 4, 5 and 6 distinct tables (kSlotsPerSet is 6)."""
    n = {hc.distinct_tables(c.huff, len(c.factors)) for c in hc.all_cases()}
    assert {2, 3, 4, 5, 6} <= n and max(n) == 6
    assert {hc.distinct_tables(c.huff, 3) for c in hc.family_cases("six") if c.tset.startswith("six")} == {6}
    assert {hc.distinct_tables(c.huff, 3) for c in hc.family_cases("six") if c.tset == "five" and c.layout != "gray"} == {5}


# ---------------------------------------------------------------------------------------------
# witnesses
# ---------------------------------------------------------------------------------------------
def _scan_coefs(case):
    return np.stack([case.coefs[c][row, col] for c, row, col in jd_coef.scan_blocks(case.width, case.height, case.factors)])


def _trace_coefs(d):
    """The scan's coefficients through jd_trace's canonical decoder (_symbol) and block rule (_step)."""
    t = jd_trace.parse(d)
    pattern, nmcu = jd_trace._layout(t)
    ri = t.ri or nmcu
    out = []
    for si, data in enumerate(jd_trace.segments(d, t.ecs)):
        if si * ri >= nmcu:
            break
        n = (min(si * ri + ri, nmcu) - si * ri) * len(pattern)
        val = int.from_bytes(data + b"\xff" * 16, "big")
        total = (len(data) + 16) * 8
        p = bi = k = done = 0
        pred = [0, 0, 0]
        while done < n:
            length, sym, v = jd_trace._symbol(t, pattern, val, total, p, bi, k)
            p += length
            if k == 0:
                pred[pattern[bi]] += v
                zz = np.zeros(64, np.int32)
                zz[0] = pred[pattern[bi]]
            k, fin, emit = jd_trace._step(k, sym)
            if emit is not None:
                zz[emit] = v
            if fin:
                out.append(zz)
                bi = (bi + 1) % len(pattern)
                done += 1
        assert p <= len(data) * 8 and len(data) * 8 - p < 8
    return np.stack(out)


@pytest.mark.parametrize("family", hc.FAMILIES)
def test_witnesses_agree_with_reference(family):
    bad = []
    for c in hc.family_cases(family):
        want = _scan_coefs(c)
        if c.symbols is not None:  # the reference's coefficients are what the rule makes of the symbols
            assert all(np.array_equal(jd_coef.coefs_of_symbols(*s, 0)[1:], w[1:]) for s, w in zip(c.symbols, want))
        for name, got in (("decode", jdoracle.decode(c.data)), ("decode_fast", jdoracle.decode_fast(c.data))):
            if got[0] != 0 or got[1].shape != c.ref.shape or not np.array_equal(got[1], c.ref):
                bad.append((c.id, name, got[0]))
        st, coefs = jdoracle.decode_coefs(c.data)
        if st != 0 or not np.array_equal(coefs, want):
            bad.append((c.id, "decode_coefs", st))
        if not np.array_equal(_trace_coefs(c.data), want):
            bad.append((c.id, "jd_trace"))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# the table format, restated from jd_internal.hpp
# ---------------------------------------------------------------------------------------------
def _extend(mag, size):
    return 0 if size == 0 else mag if mag >> (size - 1) else mag - (1 << size) + 1


def _decode(table, value, nbits):
    """(length, symbol) of the code at the top of the nbits-bit value, or None."""
    for length in range(1, nbits + 1):
        sym = table.get((length, value >> (nbits - length)))
        if sym is not None:
            return length, sym
    return None


def _rare_entry(length, sym, is_dc):
    """The 20-bit symbol entry: L 0..4, sz16 5, emit 6, adv 8..14, dc 15, sz 16..19; 0: unrepresentable."""
    size = sym if is_dc else sym & 15
    if size > 16 or length + size > 31:
        return 0
    if is_dc:
        return (length + size) | (1 << 15) | ((size & 15) << 16) | ((size >> 4) << 5)
    adv = 64 if sym == 0 else (sym >> 4) + 1
    return (length + size) | ((1 << 6) if size else 0) | (adv << 8) | (size << 16)


Entry = collections.namedtuple("Entry", "rare e L1 adv1 dc E1 w1 M1 P E2 adv2 L12 v2 size1 sym1 sym2")


@functools.lru_cache(None)
def _lut_model_cached(bits, vals, is_dc):
    table = {(length, code): sym for sym, code, length in hc.codes_of((bits, vals))}
    out = []
    for idx in range(1 << LUT_BITS):
        got = _decode(table, idx, LUT_BITS)
        e = _rare_entry(*got, is_dc) if got else 0
        size = (got[1] if is_dc else got[1] & 15) if got else 0
        if e == 0 or size >= (12 if is_dc else 10):
            out.append(Entry(True, e, *([0] * 11), size, got[1] if got else None, None))
            continue
        length, sym = got
        L1 = length + size
        adv1 = 0 if is_dc else 64 if sym == 0 else (sym >> 4) + 1
        if L1 <= LUT_BITS:  # the index holds the magnitude: the value itself
            w1, M1 = 0, -_extend((idx >> (LUT_BITS - L1)) & ((1 << size) - 1), size)
        else:
            w1, M1 = size, (1 << size) - 1
        P = E2 = adv2 = L12 = v2 = 0
        sym2 = None
        rest = LUT_BITS - L1  # index bits after the first symbol
        if not is_dc and sym != 0 and rest > 0:
            nxt = _decode(table, idx & ((1 << rest) - 1), rest)
            if nxt and nxt[0] + (nxt[1] & 15) <= rest:
                l2, sym2 = nxt
                s2 = sym2 & 15
                P, E2, adv2, L12 = 1, int(s2 > 0), 64 if sym2 == 0 else (sym2 >> 4) + 1, L1 + l2 + s2
                v2 = _extend((idx >> (LUT_BITS - L12)) & ((1 << s2) - 1), s2)
            else:
                sym2 = None
        out.append(Entry(False, 0, L1, adv1, int(is_dc), int(not is_dc and size > 0), w1, M1, P, E2, adv2, L12, v2,
                         size, sym, sym2))
    return out


def lut_model(spec, is_dc):
    return _lut_model_cached(tuple(spec[0]), tuple(spec[1]), is_dc)


def _words(en):
    """{lo, hi} of jd_internal.hpp HuffLut::fast."""
    if en.rare:
        return 1 << 15, (en.e << 12) & 0xFFFFFFFF
    lo = ((32 - en.L1) & 31) | (en.dc << 5) | (en.E1 << 6) | (en.E2 << 7) | (en.P << 8) | (en.L1 << 9) | ((en.M1 & 0xFFFF) << 16)
    hi = en.w1 | (en.adv1 << 5) | (en.adv2 << 12) | (en.L12 << 19) | ((en.v2 & 511) << 23)
    return lo, hi


def _limits(spec):
    """Annex F.2.2.3: per length (mincode, maxcode, valptr), None where the length has no code."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        n = spec[0][length - 1]
        out[length] = (code, code + n - 1, k) if n else None
        code = (code + n) << 1
        k += n
    return out


@pytest.fixture(scope="module")
def harness():
    r = subprocess.run(["make", "-C", PKG, "fuzz_host_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(PKG, "fuzz_host_asan")


def _run_harness(harness, datas, tmp_path, luts=False):
    rec = tmp_path / "records.bin"
    with open(rec, "wb") as f:
        for d in datas:
            f.write(struct.pack("<I", len(d)))
            f.write(d)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness] + (["--luts"] if luts else []) + [str(rec)], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout.strip().splitlines()


def _one_file_per_set():
    """One case of every table set: the first with the most components."""
    best = {}
    for c in hc.all_cases():
        if c.tset not in best or len(c.factors) > len(best[c.tset].factors):
            best[c.tset] = c
    return list(best.values())


def test_build_lut_every_entry(harness, tmp_path):
    """All 1024 {lo, hi} entries, lim[] and base[] of every table of every family, as the host
    harness prints them, against the model."""
    cases = _one_file_per_set()
    lines = iter(_run_harness(harness, [c.data for c in cases], tmp_path, luts=True))
    bad, tables = [], set()
    for c in cases:
        assert next(lines).split() == ["0", str(len(c.factors))]
        for comp in range(len(c.factors)):
            for ac in (0, 1):
                w = next(lines).split()
                assert w[:4] == ["lut", str(comp), str(ac), "1"], w[:4]
                words = [int(x, 16) for x in w[4:]]
                assert len(words) == 2048 + 40
                spec = c.huff["tables"][comp][ac]
                tables.add((ac, tuple(spec[0]), tuple(spec[1])))
                model = lut_model(spec, not ac)
                for idx, en in enumerate(model):
                    if _words(en) != (words[2 * idx], words[2 * idx + 1]):
                        bad.append((c.tset, comp, ac, idx, en, hex(words[2 * idx]), hex(words[2 * idx + 1])))
                lim, base = words[2048:2068], words[2068:2088]
                prev = 0
                for length, mmv in _limits(spec).items():
                    if mmv is None:
                        ok = lim[length] == prev  # no code of this length: the limit of the shorter ones
                    else:
                        ok = lim[length] == (mmv[1] + 1) << (16 - length) and base[length] == (mmv[2] - mmv[0]) & 0xFFFFFFFF
                    prev = lim[length]
                    if not ok:
                        bad.append((c.tset, comp, ac, "lim/base", length))
                if lim[17] != 0xFFFFFFFF or lim[19] != 1 - ac:
                    bad.append((c.tset, comp, ac, "lim[17]/lim[19]"))
    assert len(tables) >= 30  # the distinct tables of the families
    assert not bad, (len(bad), bad[:5])


# ---------------------------------------------------------------------------------------------
# coverage audit: which index entries a walk of each stream meets
# ---------------------------------------------------------------------------------------------
def _audit(case):
    """Counter of (class, 'Y' | 'C') over the stream's symbols, from the tables and the bit string
    alone: at every symbol the next 10 bits index the model; an entry that holds a pair consumes
    both symbols when the first leaves the block open (z + adv1 < 63), as the piece walks do."""
    t = jd_trace.parse(case.data)
    nc = len(case.factors)
    eff = [(1, 1)] if nc == 1 else case.factors
    pattern = [c for c in range(nc) for _ in range(eff[c][0] * eff[c][1])]
    nmcu = len(jd_coef.scan_blocks(case.width, case.height, case.factors)) // len(pattern)
    ri = case.restart or nmcu
    full = [[{(length, code): sym for sym, code, length in hc.codes_of(case.huff["tables"][c][tc])} for tc in (0, 1)]
            for c in range(nc)]
    models = [[lut_model(case.huff["tables"][c][tc], tc == 0) for tc in (0, 1)] for c in range(nc)]
    seen = collections.Counter()
    for si, data in enumerate(jd_trace.segments(case.data, t.ecs)):
        n = (min(si * ri + ri, nmcu) - si * ri) * len(pattern)
        val = int.from_bytes(data + b"\xff" * 8, "big")
        total = (len(data) + 8) * 8
        p = blk = z = 0
        at_dc = True
        while blk < n:
            comp = pattern[blk % len(pattern)]
            where = "Y" if comp == 0 else "C"
            tc = 0 if at_dc else 1
            what = "dc" if at_dc else "ac"
            en = models[comp][tc][(val >> (total - p - LUT_BITS)) & ((1 << LUT_BITS) - 1)]
            hit = []
            if en.rare:
                length, sym = _decode(full[comp][tc], (val >> (total - p - 16)) & 0xFFFF, 16)
                size = sym if at_dc else sym & 15
                if length > LUT_BITS:
                    hit.append(f"long-{what}-{length}")
                if size >= (12 if at_dc else 10):
                    hit.append(f"rare-{what}-size{size}")
                    if length == 1 or (at_dc and length <= LUT_BITS):
                        hit.append(f"rare-{what}-size{size}-code{'1' if length == 1 else '<=10'}")
                p += length + size
                adv = 0 if at_dc else 64 if sym == 0 else (sym >> 4) + 1
                zn = z + adv
                if not at_dc and sym & 15 and zn > 63:
                    hit.append("first-past-63-dropped")
                if not at_dc and sym and not sym & 15 and sym != 0xF0:
                    hit.append(f"size0-run{sym >> 4}")
            else:
                hit.append("resolved" if en.w1 == 0 else f"beyond-{what}-size{en.size1}")
                code = en.L1 - en.size1
                if code == LUT_BITS:  # the code fills the index: nothing of the magnitude within it
                    hit.append(f"code10-{what}-" + ("size0" if en.size1 == 0 else "beyond"))
                if not at_dc and en.L1 == LUT_BITS and code <= 3:
                    hit.append("short-code-fills-index" + ("-size9-code1" if code == 1 else ""))
                zn = z + en.adv1
                if en.E1 and zn > 63:
                    hit.append("first-past-63-dropped")
                if not at_dc and en.sym1 and not en.sym1 & 15 and en.sym1 != 0xF0:
                    hit.append(f"size0-run{en.sym1 >> 4}")
                if en.P and zn < 63:
                    s2 = en.sym2
                    hit.append("pair-eob" if s2 == 0 else "pair-zrl" if s2 == 0xF0 else f"pair-size{s2 & 15}")
                    if s2 & 15 == 8 and abs(en.v2) in (128, 255):
                        hit.append(f"v2={en.v2}")
                    if en.L12 == LUT_BITS:
                        hit.append("L12=10")
                    zn += en.adv2
                    if s2 and zn == 63:
                        hit.append("pair-second-lands-on-63")
                    if s2 and zn > 63:
                        hit.append("pair-second-past-63")
                    p += en.L12
                else:
                    if en.P:
                        hit.append("pair-entry-at-block-end")  # the bits after the first symbol: the next DC
                    p += en.L1
            for h in hit:
                seen[(h, where)] += 1
            at_dc = False
            z = zn
            if zn >= 63:
                blk, z, at_dc = blk + 1, 0, True
        assert p <= len(data) * 8 and len(data) * 8 - p < 8, case.id  # the model's walk is the stream's
    return seen


@functools.lru_cache(None)
def _audits():
    return {c.id: _audit(c) for c in hc.all_cases()}


CLASSES = (["code10-ac-size0", "code10-ac-beyond", "code10-dc-beyond", "short-code-fills-index",
            "short-code-fills-index-size9-code1", "rare-ac-size10-code1", "rare-dc-size12-code<=10", "resolved", "beyond-ac-size9", "beyond-dc-size11", "L12=10", "pair-eob", "pair-zrl", "pair-entry-at-block-end",
            "pair-second-lands-on-63"] + [f"rare-ac-size{s}" for s in range(10, 16)] +
           [f"rare-dc-size{s}" for s in range(12, 17)] + [f"long-{w}-{l}" for w in ("dc", "ac") for l in range(11, 17)] +
           [f"pair-size{s}" for s in range(1, 9)] + [f"v2={v}" for v in (-255, -128, 128, 255)])
SYMBOL_CLASSES = ["first-past-63-dropped", "pair-second-past-63"] + [f"size0-run{r}" for r in range(1, 15)]


def _totals(cases):
    tot = collections.Counter()
    for c in cases:
        tot.update(_audits()[c.id])
    return tot


def _missing(cases):
    plain = _totals(c for c in cases if c.symbols is None)
    sym = _totals(c for c in cases if c.symbols is not None)
    return ([(k, w) for k in CLASSES for w in "YC" if not plain[(k, w)]] +
            [(k, w) for k in SYMBOL_CLASSES for w in "YC" if not sym[(k, w)]])


def test_coverage_audit():
    """Every class of index entry is met at least once in a luma and once in a chroma position of a
    coefficient-level case (the last two groups: of a symbol-level case, no coefficients produce
    them).  'pair-second-lands-on-63' is the coefficient-level form of a pair whose second symbol
    ends the block; past 63 it is symbol-level."""
    assert _missing(hc.all_cases()) == []
    tot = _totals(hc.all_cases())
    print({k: (tot[(k, "Y")], tot[(k, "C")]) for k in CLASSES + SYMBOL_CLASSES})
    # the symbol-level classes do not occur in coefficient-level cases: those are what encoders write
    plain = _totals(c for c in hc.all_cases() if c.symbols is None)
    assert not any(plain[(k, w)] for k in SYMBOL_CLASSES for w in "YC")


def test_uniform_streams_have_no_short_codes():
    """uniform: with every code of 11 (15/16) bits no symbol is served by the index, with every code
    of 10 bits every symbol is and none holds a pair or any of its magnitude."""
    for c in hc.family_cases("uniform"):
        kinds = {k.split("-size")[0] for k, _ in _audits()[c.id]}
        if c.tset == "uni10":
            assert kinds <= {"resolved", "beyond-ac", "beyond-dc", "code10-ac", "code10-dc", "code10-ac-beyond",
                             "code10-dc-beyond", "rare-ac", "rare-dc"}, kinds
            assert not any(k.startswith(("long", "pair", "L12")) for k in kinds)
            assert _audits()[c.id][("resolved", "Y")] == sum(n for (k, w), n in _audits()[c.id].items()
                                                             if w == "Y" and k.endswith("-size0") and k.startswith("code10"))
        else:
            assert kinds and all(k.startswith(("long-", "rare-")) for k in kinds), kinds
            lengths = {int(k.split("-")[2]) for k in kinds if k.startswith("long-")}
            assert lengths == ({11} if c.tset == "uni11" else {15, 16})


@pytest.mark.parametrize("family", ["stair", "edge", "pairs"])
def test_coverage_needs_the_family(family):
    """Without the family at least one class is not met (uniform, dense, six and ident are there
    for what the other tests assert: no short codes, the pools, the slots and the cache key)."""
    assert _missing([c for c in hc.all_cases() if c.family != family]) != []


# ---------------------------------------------------------------------------------------------
# region_divisor against the densest block
# ---------------------------------------------------------------------------------------------
def test_region_divisor_is_the_densest_block(harness, tmp_path):
    """rw_div (jd_plan.cpp region_divisor, the harness's field 13) against hc.true_divisor(): a DP
    over the coefficient index that maximises d x words - bits over every block the tables allow.
    Safety is rw_div <= the truth; equality says the three shapes region_divisor looks at are the
    extremes, which holds where the cheapest entry symbol has a long run or an EOB block is denser
    anyway (every set but one).  The dense family reaches every value 2..8."""
    cases = _one_file_per_set()
    out = [[int(x) for x in ln.split()] for ln in _run_harness(harness, [c.data for c in cases], tmp_path)]
    got = {c.tset: o[13] for c, o in zip(cases, out)}
    want = {c.tset: hc.true_divisor(c.huff, len(c.factors)) for c in cases}
    print(got, want)
    assert all(o[0] == 0 and o[9] == 0 for o in out)
    assert all(got[t] <= want[t] for t in got), (got, want)
    # One family set is loose, for the reason spelt out below: IDENT_A's cheapest entry is 0x01 (run 0, 3
    # bits), and four of those do not reach position 63; the real densest block is DC + EOB (5 bits).
    loose = {"dc10-dc": (4, 5)}
    assert {t: (got[t], want[t]) for t in got if got[t] != want[t]} == loose
    assert [got[f"dense{d}"] for d in range(2, 9)] == list(range(2, 9))
    # Where the bound is loose: region_divisor takes a block without EOB for four AC
    # symbols of the fewest bits, each an entry.  Here that symbol is 0xF1 (run 15): only three of
    # them land inside the block (16, 32, 48), the fourth is read and dropped, so the densest block
    # is 2.5 words in 10 bits (4) where region_divisor assumes 3 words (3): safe, one step small.
    dc = {0: 2}
    dc.update({s: 8 for s in range(1, 12)})
    ac = {0xF1: 1, 0x00: 8, 0x01: 8, 0x02: 9}
    huff = {"tables": [(jd_coef.canonical(dc), jd_coef.canonical(ac))], "ids": [(0, 0)], "packing": "each"}
    data = jd_coef.build(8, 8, [(1, 1)], [np.zeros((1, 1, 64), np.int32)], [hc.UNIT], huff=huff)
    loose = int(_run_harness(harness, [data], tmp_path)[0].split()[13])
    assert (loose, hc.true_divisor(huff, 1)) == (3, 4)
