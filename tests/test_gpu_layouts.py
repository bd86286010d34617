"""GPU parity on every sampling layout and quantisation range the parser accepts.

Inputs: tests/layout_cases.py, built from chosen coefficients by tools/jd_coef.py (the CPU file
tests/test_layouts_ref.py audits what they cover).  References: jd_coef's plain reference() of
the same coefficients, and jdoracle.decode as a second witness (the two agree on every case, CPU
test).  Each test decodes its cases in one batch on each entropy path (the `decoder` fixture).
Bar: status 0 and bit-exact RGB.
"""
import numpy as np
import pytest

import jdamd
import layout_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fancy_decoder():
    dec = jdamd.Decoder(0, timing=True, fancy=True)
    yield dec
    dec.close()


def _mismatches(dec, cases, fancy=False):
    outs, status = dec.decode_batch([c.data for c in cases])
    oracle = lc.oracle_outputs(fancy)
    bad = []
    for c, o, s in zip(cases, outs, status):
        refs = [oracle[c.id][1]] if fancy else [c.ref, oracle[c.id][1]]
        assert oracle[c.id][0] == 0
        if s != 0 or any(o.shape != r.shape or not np.array_equal(o, r) for r in refs):
            diff = None
            if s == 0 and o.shape == refs[0].shape:
                d = np.abs(o.astype(int) - refs[0].astype(int))
                diff = (int((d > 0).any(-1).sum()), int(d.max()))  # pixels off, largest difference
            bad.append((c.id, s, diff))
    return bad


def test_layout_matrix(decoder):
    """16 layouts x (5 x 3, a two-tile image without / with 1-MCU / with odd restart intervals),
    random dense coefficients: the generic instance's cmode 2 and 4 branches, vertical shifts of
    2, hc = 4, luma below the maximum factor."""
    assert _mismatches(decoder, lc.matrix_cases()) == []


def test_layout_matrix_fancy(fancy_decoder):
    """The same files with fancy upsampling (per-pixel fancy_win for the unusual layouts)."""
    assert _mismatches(fancy_decoder, lc.matrix_cases(), fancy=True) == []


def test_colour_directed(decoder):
    """Exact-class chroma pairs and clamped channels at every pixel position of every layout's
    colour path (terms_il, fix_g_exact, colour4x1 / colour4x2, load8_samples), all store tails."""
    assert _mismatches(decoder, lc.colour_cases()) == []


def test_quant_range(decoder):
    """8- and 16-bit tables with largest steps from 1 to 65535, coefficients on both sides of the
    fast IDCT form's range test, of the entry slots' escape edge and of int16 after
    dequantisation: fast and exact tiles side by side in every image."""
    assert _mismatches(decoder, lc.quant_cases()) == []


def test_many_entries(decoder):
    """Blocks of 0 .. 63 non-zero ACs starting at varied entry offsets, with and without escaped
    values (load_entry_quads, the quad loop beyond the prefetch, scatter_quad's masks)."""
    assert _mismatches(decoder, lc.entry_cases()) == []
