"""GPU parity over the Huffman table space.

Inputs: tests/huff_cases.py, built by tools/jd_coef.py from chosen coefficients (or symbols) and
chosen table sets; the CPU file tests/test_huff_ref.py audits what they cover, checks build_lut
entry by entry and settles the witnesses.  References: jd_coef's reference() of the same
coefficients (it never sees a table), and jdoracle.decode as a second witness.  Each family is
decoded in one batch on each entropy path (the `decoder` fixture).  Bar: status 0 and bit-exact RGB.
"""
import numpy as np
import pytest

import huff_cases as hc
import jdamd

pytestmark = pytest.mark.gpu


def _mismatches(outs, status, cases):
    """(id, status, (pixels off, largest difference)) of every case that is not bit-exact."""
    oracle = hc.oracle_outputs()
    bad = []
    for c, o, s in zip(cases, outs, status):
        assert oracle[c.id][0] == 0
        refs = [c.ref, oracle[c.id][1]]
        if s != 0 or any(o.shape != r.shape or not np.array_equal(o, r) for r in refs):
            diff = None
            if s == 0 and o.shape == refs[0].shape:
                d = np.abs(o.astype(int) - refs[0].astype(int))
                diff = (int((d > 0).any(-1).sum()), int(d.max()))
            bad.append((c.id, s, diff))
    return bad


def _decode(dec, cases):
    return _mismatches(*dec.decode_batch([c.data for c in cases]), cases)


@pytest.mark.parametrize("family", hc.FAMILIES)
def test_family(decoder, family):
    """stair: codes of every length, every size behind long codes, the symbol sequences no
    coefficients produce.  edge: 9-, 10- and 11-bit codes, l + size = 10.  uniform: no short
    codes.  pairs: two symbols per index entry.  dense: 2 .. 8 walk bits per region word.  six:
    six and five LUT slots, permuted DHT ids, every DHT packing.  ident: the LUT cache's key."""
    assert _decode(decoder, hc.family_cases(family)) == []


def test_all_families_one_batch_then_reversed(decoder):
    """Many table sets and slot counts 2 .. 6 in one launch; then the same files in reverse order on
    the same decoder, every LUT now served from the cache."""
    cases = hc.all_cases()
    assert _decode(decoder, cases) == []
    assert _decode(decoder, cases[::-1]) == []


def test_lut_cache_identity():
    """One decoder, one file per call, then all in one batch: tables of equal counts and permuted
    values; of equal values and other counts; of the same bytes as a DC and as an AC table, across
    calls (ident) and within one frame (six: Cb's AC table is its DC table's bytes)."""
    cases = hc.family_cases("ident") + [c for c in hc.family_cases("six") if c.tset == "six-each"]
    dec = jdamd.Decoder(0)
    try:
        for c in cases:
            assert _decode(dec, [c]) == [], c.id
        assert _decode(dec, cases[::-1]) == []
    finally:
        dec.close()


@pytest.mark.parametrize("path", ["auto", "sync", "lanes", "full"])
def test_dense_streams_and_pools(path):
    """The dense family (its densest blocks fill one region word per 2 .. 8 walk bits: the worst
    case region_divisor sizes the pools for) with worst-case pools decodes without a retry; with
    the default pools it is bit-exact whether or not an image was decoded twice."""
    cases = hc.family_cases("dense")
    for worst in (True, False):
        dec = jdamd.Decoder(0, path=path, worst_case_pools=worst)
        try:
            assert _decode(dec, cases) == []
            if worst:
                assert dec.stats()["retried_images"] == 0
        finally:
            dec.close()


def test_pipelined_batches_bring_new_tables():
    """jd_decode_batch_async: every batch carries table sets the context has not seen, so the
    device LUT array is re-uploaded (and grows) while the previous batch is in flight."""
    batches = [[c for c in hc.family_cases(f) if c.width < 1024] for f in hc.FAMILIES]
    dec = jdamd.Decoder(0)
    try:
        runs = []
        for cases in batches:
            hosts = [np.frombuffer(c.data, np.uint8).copy() for c in cases]
            ooffs, tot = [], 0
            for c in cases:
                ooffs.append(tot)
                tot += (c.width * c.height * 3 + 255) // 256 * 256
            dout = dec.alloc(tot)
            bt = dec.make_batch(hosts, [None] * len(cases), [dout.ptr + o for o in ooffs])
            dec.decode_prepared(bt, pipelined=True)
            runs.append((cases, hosts, bt, dout, ooffs))
        dec.wait()
        for cases, _, bt, dout, ooffs in runs:
            outs = [dout.download(np.empty((c.height, c.width, 3), np.uint8), o) for c, o in zip(cases, ooffs)]
            assert _mismatches(outs, [r.status for r in bt[1]], cases) == []
    finally:
        dec.close()


def test_dc_size16_behind_a_16_bit_code_is_corrupt(decoder):
    """The one known deviation from the oracle's status: code + magnitude of 32 bits
    do not fit the device symbol entry (jd_internal.hpp lut_entry: 5 bits of length, a 32-bit
    peek), so the slow path reports the symbol as a bad code.  The oracle decodes the file, to the
    reference's pixels (tests/test_huff_ref.py)."""
    case = hc.dc16_case()
    outs, status = decoder.decode_batch([case.data])
    assert status == [jdamd.JD_ERR_CORRUPT] and outs == [None]
