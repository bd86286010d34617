"""CPU: the oracle against a plain reference on every sampling layout and quantisation range the
parser accepts, and the coverage audits of the directed inputs.

Reference: tools/jd_coef.py reference() — the coefficients a test chose, dequantised, through
jdoracle.idct (pinned to the reference decoder by the ground-truth fixtures), replicate-upsampled
by index arithmetic and coloured in float64 / float32 as tests/test_gpu.py::test_color_exhaustive
does.  It reads no bitstream and shares no layout or colour code with oracle/jdoracle.c.  Bar:
bit-exact.  The same cases run on the GPU in tests/test_gpu_layouts.py; the audits below are
conditions on those inputs (computed from the reference's planes alone), not tolerances.
"""
import os
import tempfile

import numpy as np
import pytest

import jdoracle
import layout_cases as lc

import jd_coef  # noqa: E402  (tools/ is on the path once layout_cases is imported)


def _check(cases):
    got = lc.oracle_outputs()
    bad = []
    for c in cases:
        st, px = got[c.id]
        if st != 0 or px.shape != c.ref.shape or not np.array_equal(px, c.ref):
            bad.append((c.id, st, None if px is None else int((px != c.ref).any(-1).sum())))
    assert not bad, bad


def test_huffman_tables_are_annex_k():
    """The builder's tables are the encoder's (Annex K.3), the DC one extended by symbol 12."""
    src = open(os.path.join(lc.ROOT, "tools", "jdenc.c")).read()

    def table(name):
        body = src.split(name)[1].split("{", 1)[1].split("}", 1)[0]
        return [int(x, 0) for x in body.replace("\n", " ").split(",") if x.strip()]

    assert jd_coef.AC_LUMA_BITS == table("kAcLumaBits[16] =") and jd_coef.AC_LUMA_VALS == table("kAcLumaVals[162] =")
    assert jd_coef.AC_CHROMA_BITS == table("kAcChromaBits[16] =")
    assert jd_coef.AC_CHROMA_VALS == table("kAcChromaVals[162] =")
    assert jd_coef.ZIGZAG == table("kZigzag[64] =")
    bits = table("kDcLumaBits[16] =")
    bits[9] += 1
    assert jd_coef.DC_BITS == bits and jd_coef.DC_VALS == table("kDcVals[12] =") + [12]


def test_builder_round_trips_coefficients():
    """Every coefficient of every case comes back from the oracle's entropy decoder (scan order)."""
    for c in lc.matrix_cases()[:8] + lc.quant_cases()[:3] + lc.entry_cases()[:2]:
        st, got = jdoracle.decode_coefs(c.data)
        assert st == 0
        g = lc.geometry(c.layout)
        _, _, mcux, mcuy = jd_coef.grid(c.width, c.height, c.factors)
        want = []
        for m in range(mcux * mcuy):
            my, mx = divmod(m, mcux)
            for k, (h, v) in enumerate(g.eff):
                want += [c.coefs[k][my * v + by, mx * h + bx] for by in range(v) for bx in range(h)]
        assert np.array_equal(got, np.stack(want)), c.id


def test_layout_table_is_the_issue_s():
    """Blocks per MCU of the unusual layouts, and the sizes: 5 x 3 and one of more than one tile
    whose last 8-pixel group and last row pair are partial."""
    bpm = {n: lc.geometry(n).bpm for n in lc.LAYOUTS}
    assert [bpm[n] for n in list(lc.LAYOUTS)[:11]] == [6, 10, 6, 10, 5, 8, 5, 7, 6, 5, 6]
    for n in lc.LAYOUTS:
        g = lc.geometry(n)
        cs = [c for c in lc.matrix_cases() if c.layout == n]
        assert [(c.width, c.height) for c in cs] == [(5, 3)] + [(g.width, g.height)] * 3
        assert g.width > 8 * g.hmax * g.tile_mcus and g.width % 8 == 5 and g.height % 2 == 1
        assert g.width < 500 and g.height < 64
        assert [c.restart for c in cs][1:3] == [0, 1] and g.tile_mcus % cs[3].restart != 0


def test_oracle_matches_reference_layout_matrix():
    _check(lc.matrix_cases())


def test_oracle_matches_reference_colour_directed():
    _check(lc.colour_cases())


def test_oracle_matches_reference_quant_range():
    _check(lc.quant_cases())


def test_oracle_matches_reference_many_entries():
    _check(lc.entry_cases())


def test_exact_class_pairs():
    """54 of the 2^18 (Cb, Cr) pairs take the double-precision G patch."""
    pairs = lc.exact_pairs()
    assert len(pairs) == 54 and (-203, -17) in pairs and (-200, 200) in pairs


@pytest.mark.parametrize("case", lc.colour_cases(), ids=lambda c: c.id)
def test_colour_inputs_cover_every_position(case):
    g = lc.geometry(case.layout)
    assert case.height % 2 == 1
    # every cell (x mod 8, y mod MCU height): an exact-class pixel, each channel at 0 and at 255
    assert lc.cell_audit(case, 8 * g.vmax) == []
    # every position of an 8-pixel group: exact-class among non-exact ones, and the reverse
    ex = jd_coef.exact_class(case.ycc[1], case.ycc[2])
    assert lc.group_audit(ex) == ([True] * 8, [True] * 8)
    # the tile tails (colour4x1: rows 6-7 of each 8-row band; colour4x2: rows 12-15 of each 16)
    if case.layout == "4:4:4":
        assert lc.group_audit(ex, {6, 7}, 8) == ([True] * 8, [True] * 8)
    if case.layout == "4:2:0":
        assert lc.group_audit(ex, {12, 13, 14, 15}, 16) == ([True] * 8, [True] * 8)
    # Y at both clip limits under an exact-class chroma pair
    y = case.ycc[0]
    assert (ex & (y == -256)).any() and (ex & (y == 255)).any()


def test_colour_inputs_cover_every_store_tail():
    assert {c.width % 8 for c in lc.colour_cases()} == {1, 3, 4, 7}
    assert [c.layout for c in lc.colour_cases()] == lc.COLOUR_LAYOUTS


@pytest.mark.parametrize("case", lc.quant_cases(), ids=lambda c: c.id)
def test_quant_inputs_straddle_int16(case):
    qv, q = case.qv, case.qmax
    assert max(max(t) for t in case.qtabs) == q
    deq = np.concatenate([d.ravel() for d in jd_coef.dequantised(case.coefs, case.qtabs)]).astype(np.int64)
    inside = (deq >= -32768) & (deq <= 32767)
    assert inside.any()
    # (a step of 1 cannot leave int16: the largest coefficient the tables code is 2047)
    assert (~inside).any() == (q > 1)
    if q > 16:
        edges = [(32767 // q) * q, (32767 // q + 1) * q, -(32768 // q) * q, -(32768 // q + 1) * q]
        assert all((deq == e).any() for e in edges), edges
    # every listed value is present, at the first, the last and a middle zig-zag position
    ac = np.concatenate([c[..., 1:].reshape(-1, 63) for c in case.coefs])
    for v in qv.ac_in + qv.ac_mid + qv.ac_out:
        assert (ac == v).any(), v
    for p in lc.QUANT_POS:
        assert (ac[:, p - 1] != 0).any(), p
    k = lc.fast_k(q)
    want = {-1, 1, 511, -511, 512, -512, 513, -513, 1023, -1023}
    if k:
        want |= {v for v in (-(1 << (k - 1)), -(1 << (k - 1)) - 1, (1 << (k - 1)) - 1, 1 << (k - 1)) if v}
    assert {v for v in want if abs(v) <= 1023} == set(qv.ac_in + qv.ac_mid + qv.ac_out)
    # natural row 7 (zig-zag 35 and 63 among the positions used) empty in some blocks, not in others
    r7 = (ac[:, 34] != 0) | (ac[:, 62] != 0)
    if qv.ac_in:
        assert r7.any() and (~r7).any()
    # per MCU row after the first: exactly one block out of the fast form's range, in the first tile
    # (the second tile of every row, and all of row 0, hold none: the fast form runs there)
    g = lc.geometry(case.layout)
    out_rows = 0
    for c, a in enumerate(case.coefs):
        h, v = g.eff[c]
        dc = a[..., 0].astype(np.int64) * case.qtabs[0 if c == 0 else 1][0]
        lim = (1 << (k - 1)) if k else 0
        ac_out = (a[..., 1:] != 0) if k == 0 else ((a[..., 1:] < -lim) | (a[..., 1:] >= lim))
        out = (dc < -32768) | (dc > 32767) | ac_out.any(-1)
        assert not out[:v].any() and not out[:, g.tile_mcus * h:].any()
        out_rows = out_rows + out.reshape(-1, v, out.shape[1]).sum((1, 2))
    assert out_rows.tolist() == [0] + [1] * (len(out_rows) - 1)


def test_entry_inputs_cover_counts_and_offsets():
    """Every listed count of non-zero ACs, each starting at several offsets mod 8 of the running
    entry count (the stand-in on the CPU for the decoder's entry_start & 7)."""
    for case in lc.entry_cases():
        cnt = np.array(case.counts)
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]]) & 7
        listed = np.arange(cnt.size) % 2 == 1
        for n in lc.ENTRY_COUNTS:
            assert len(set(start[listed & (cnt == n)].tolist())) >= 4, (case.id, n)
        nz = np.concatenate([(c[..., 1:] != 0).sum(-1).ravel() for c in case.coefs])
        assert set(lc.ENTRY_COUNTS) <= set(nz.tolist())


@pytest.mark.skipif(not jdoracle.ref_available(), reason="oracle/_ref/decoder not built")
def test_reference_decoder_reads_builder_444():
    """A 4:4:4 unit-quant file of the builder through the reference decoder itself."""
    case = next(c for c in lc.colour_cases() if c.layout == "4:4:4")
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "coef444.jpg")
        with open(p, "wb") as f:
            f.write(case.data)
        assert np.array_equal(jdoracle.ref_decode(p, td), case.ref)
