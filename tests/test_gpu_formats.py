"""GPU parity of the output formats: planar, BGR, planar BGR and gray (JD_FLAG_OUT_*).

References come from outside the decoder (tests/format_cases.py): numpy permutations of jd_coef's
plain reference and of jdoracle.decode, and the luma plane clip(Y + 128, 0, 255).  The CPU file
tests/test_formats_abi.py audits the gray reference.  Bar everywhere: status 0 and bit-exact bytes.
"""
import ctypes

import numpy as np
import pytest

import format_cases as fc
import jdamd
import jdoracle
import layout_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def decoders():
    """One decoder per format (default entropy path), and the fancy ones, made on first use."""
    made = {}

    def get(fmt, fancy=False):
        if (fmt, fancy) not in made:
            layout, channels = fc.FORMATS[fmt]
            made[(fmt, fancy)] = jdamd.Decoder(0, timing=True, fancy=fancy, layout=layout, channels=channels)
        return made[(fmt, fancy)]

    yield get
    for d in made.values():
        d.close()


def _mismatches(dec, cases, fmt, refs_of):
    """One host-output batch of all the cases; refs_of(case) -> list of references."""
    outs, status = dec.decode_batch([c.data for c in cases])
    bad = []
    for c, o, s in zip(cases, outs, status):
        refs = refs_of(c)
        if s != 0 or o.shape != dec.output_shape(c.height, c.width) or any(
                o.shape != r.shape or not np.array_equal(o, r) for r in refs):
            diff = None
            if s == 0 and o.shape == refs[0].shape:
                d = np.abs(o.astype(int) - refs[0].astype(int))
                diff = (int((d > 0).sum()), int(d.max()))  # bytes off, largest difference
            bad.append((c.id, s, diff))
    return bad


def _plain_refs(fmt):
    oracle = lc.oracle_outputs(False)

    def refs(c):
        if fmt == "gray":
            return [fc.gray_of_case(c)]
        assert oracle[c.id][0] == 0
        return [fc.permuted(c.ref, fmt), fc.permuted(oracle[c.id][1], fmt)]

    return refs


@pytest.mark.parametrize("fmt", list(fc.FORMATS))
def test_layout_matrix(decoders, fmt):
    """16 layouts x four sizes in one batch, so every layout instance of the format launches: the
    generic instance's cmode 2, 3 and 4 branches, luma below the maximum factor, full first tiles
    (the 4-pixel-halves steps)."""
    assert _mismatches(decoders(fmt), lc.matrix_cases(), fmt, _plain_refs(fmt)) == []


@pytest.mark.parametrize("fmt", fc.COLOUR_FORMATS)
def test_colour_directed(decoders, fmt):
    """Exact-class chroma pairs and clamped channels at every pixel position of every group, tails
    included: a G patch written to the wrong byte shows here."""
    assert _mismatches(decoders(fmt), lc.colour_cases(), fmt, _plain_refs(fmt)) == []


@pytest.mark.parametrize("fmt", list(fc.FORMATS))
def test_quant_range_both_idct_forms(decoders, fmt):
    """Fast and exact tiles side by side: k_idct_color_exact writes each format too."""
    assert _mismatches(decoders(fmt), lc.quant_cases(), fmt, _plain_refs(fmt)) == []


@pytest.mark.parametrize("fmt", fc.COLOUR_FORMATS)
def test_fancy(decoders, fmt):
    """k_colour_fancy's vectorised and per-pixel stores, against jdoracle.decode(fancy=True) permuted."""
    cases = lc.matrix_cases() + lc.colour_cases()
    fancy_ref = {c.id: jdoracle.decode(c.data, fancy=True) for c in lc.colour_cases()}
    fancy_ref.update(lc.oracle_outputs(True))

    def refs(c):
        assert fancy_ref[c.id][0] == 0
        return [fc.permuted(fancy_ref[c.id][1], fmt)]

    assert _mismatches(decoders(fmt, fancy=True), cases, fmt, refs) == []


def test_gray_ignores_fancy(decoders):
    """Gray never runs the fancy path: byte for byte the output without the flag, no k_colour_fancy."""
    cases = lc.matrix_cases()
    dec = decoders("gray", fancy=True)
    dec.reset_stats()
    assert _mismatches(dec, cases, "gray", _plain_refs("gray")) == []
    plain, _ = decoders("gray").decode_batch([c.data for c in cases])
    fancy, _ = dec.decode_batch([c.data for c in cases])
    assert all(np.array_equal(a, b) for a, b in zip(plain, fancy))
    assert dec.stats()["kernels"]["k_colour_fancy"]["launches"] == 0


def test_stats_count_written_bytes(decoders):
    """jd_get_stats' algorithmic bytes of k_idct_color count what the format writes: the same for
    every 3-channel format, two bytes per pixel fewer for gray."""
    c = lc.matrix_cases()[-5]
    nbytes = {}
    for fmt in fc.FORMATS:
        dec = decoders(fmt)
        dec.reset_stats()
        dec.decode(c.data)
        nbytes[fmt] = dec.stats()["kernels"]["k_idct_color"]["bytes"]
    assert nbytes["chw"] == nbytes["bgr"] == nbytes["chw-bgr"]
    assert nbytes["bgr"] - nbytes["gray"] == 2 * c.width * c.height


@pytest.mark.parametrize("fmt", ["chw", "gray", "bgr"])
def test_store_alignment_and_bounds(decoders, fmt):
    """Every width 1 .. 24 at heights 1, 2 and 17 (gray, 4:4:4, 4:2:0 files), device outputs placed
    at addresses cycling through all eight residues mod 8 with 16 guard bytes between neighbours,
    in a buffer pre-filled with 0xA5: every output exact, every guard byte untouched."""
    dec = decoders(fmt)
    cases = fc.align_cases()
    offs, cur = [], 16
    for i, c in enumerate(cases):
        n = int(np.prod(dec.output_shape(c.height, c.width)))
        cur = (cur + 7) // 8 * 8 + (i % 8)
        offs.append((cur, n))
        cur += n + 16
    total = cur + 16
    buf = dec.alloc(total)
    try:
        assert buf.ptr % 8 == 0  # (so an offset's residue is its address's)
        buf.upload(np.full(total, 0xA5, np.uint8))
        hosts = [np.frombuffer(c.data, np.uint8).copy() for c in cases]
        status = dec.decode_batch_device(hosts, [None] * len(cases), [buf.ptr + o for o, _ in offs])
        assert status == [0] * len(cases)
        got = buf.download(np.empty(total, np.uint8))
    finally:
        buf.free()
    assert {(buf_off % 8) for buf_off, _ in offs} == set(range(8))
    used = np.zeros(total, bool)
    bad = []
    for c, (o, n) in zip(cases, offs):
        used[o:o + n] = True
        ref = fc.case_reference(c, fmt)
        if not np.array_equal(got[o:o + n], ref.reshape(-1)):
            bad.append(c.id)
    assert bad == []
    assert (got[~used] == 0xA5).all(), np.flatnonzero(~used & (got != 0xA5))[:16]


def test_retry_path_planar():
    """A flat 1080p image overflows the optimistic pools on the full-piece path and is decoded
    again (run_retries) with the context's flags: planar like the first launch."""
    import jd_synth

    px = np.full((1080, 1920, 3), 40, np.uint8)
    px[:, :1920 // 3] = 100  # two flat areas (as tests/test_gpu_pools.py _flat)
    data = jd_synth.encode(px, 90, "4:2:0", 0)
    dec = jdamd.Decoder(0, path="full", layout="chw")
    try:
        (out,), status = dec.decode_batch([data])
        assert status == [0]
        assert dec.stats()["retried_images"] >= 1
    finally:
        dec.close()
    assert out.shape == (3, 1080, 1920)
    assert np.array_equal(out, fc.stream_reference(data, "chw"))


def test_pipelined_batches_gray(decoders):
    """Two jd_decode_batch_async batches in flight one after the other on a gray decoder."""
    dec = decoders("gray")
    cases = lc.matrix_cases()
    halves = [cases[0::2], cases[1::2]]
    keep = []
    for part in halves:
        offs, cur = [], 0
        for c in part:
            offs.append(cur)
            cur += (c.width * c.height + 255) // 256 * 256
        buf = dec.alloc(cur)
        hosts = [np.frombuffer(c.data, np.uint8).copy() for c in part]
        bt = dec.make_batch(hosts, [None] * len(part), [buf.ptr + o for o in offs])
        dec.decode_prepared(bt, pipelined=True)
        keep.append((part, offs, cur, buf, hosts, bt))
    dec.wait()
    try:
        for part, offs, cur, buf, hosts, bt in keep:
            assert [r.status for r in bt[1]] == [0] * len(part)
            got = buf.download(np.empty(cur, np.uint8))
            for c, o in zip(part, offs):
                assert np.array_equal(got[o:o + c.width * c.height].reshape(c.height, c.width), fc.gray_of_case(c)), c.id
    finally:
        for k in keep:
            k[3].free()


@pytest.mark.parametrize("flags", [jdamd.JD_FLAG_OUT_GRAY | jdamd.JD_FLAG_OUT_PLANAR,
                                   jdamd.JD_FLAG_OUT_GRAY | jdamd.JD_FLAG_OUT_BGR])
def test_rejected_combinations(flags):
    lib = jdamd.load_library()
    ctx = ctypes.c_void_p()
    opts = jdamd._Opts(flags, 0)
    assert lib.jd_ctx_create(ctypes.byref(ctx), 0, ctypes.byref(opts)) == jdamd.JD_ERR_INVALID_ARG
    assert not ctx.value


def test_single_image_entry_points(decoders, tmp_path):
    """jd_decode and jd_decode_file size and fill their outputs by the format."""
    c = lc.matrix_cases()[-5]  # (a two-tile colour image)
    p = tmp_path / "a.jpg"
    p.write_bytes(c.data)
    for fmt in fc.FORMATS:
        dec = decoders(fmt)
        ref = fc.case_reference(c, fmt)
        assert np.array_equal(dec.decode(c.data), ref), fmt
        assert np.array_equal(dec.decode_file(str(p)), ref), fmt
