"""bench.py --dump-outputs on CPU: the files hold the images' pixel bytes only (never the alignment
gaps of the output buffer), every byte of a small batch, and the same seeded positions of a large
one from run to run."""
import collections

import numpy as np
import torch

Hdr = collections.namedtuple("Hdr", "width height")
Res = collections.namedtuple("Res", "status width height")


def _batch(fill):
    hdrs = [Hdr(5, 3), Hdr(16, 2), Hdr(7, 9)]
    offs, tot = [], 0
    for h in hdrs:
        offs.append(tot)
        tot += (h.width * h.height * 3 + 255) // 256 * 256
    buf = np.full(tot, fill, np.uint8)  # the gaps hold `fill`
    rng = np.random.default_rng(1)
    pix = [rng.integers(0, 200, h.width * h.height * 3, dtype=np.uint8) for h in hdrs]
    for o, p in zip(offs, pix):
        buf[o:o + p.size] = p
    res = [Res(0, h.width, h.height) for h in hdrs]
    return hdrs, offs, torch.from_numpy(buf), np.concatenate(pix), res


def test_dump_small_batch_is_every_pixel_byte(tmp_path):
    import bench

    hdrs, offs, buf, pix, res = _batch(255)
    bench.dump_outputs(str(tmp_path), buf, offs, hdrs, res, torch.device("cpu"))
    got = np.load(tmp_path / "rgb_sample.npy")
    assert got.dtype == np.float32 and np.array_equal(got, pix.astype(np.float32))
    r = np.load(tmp_path / "results.npy")
    assert r.dtype == np.float32 and r.tolist() == [[0, 5, 3], [0, 16, 2], [0, 7, 9]]


def test_dump_sample_is_seeded_and_skips_gaps(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    outs = []
    for run, fill in enumerate((255, 254)):  # different garbage in the gaps: same files
        hdrs, offs, buf, pix, res = _batch(fill)
        d = tmp_path / str(run)
        bench.dump_outputs(str(d), buf, offs, hdrs, res, torch.device("cpu"), suffix="_rank1")
        outs.append(np.load(d / "rgb_sample_rank1.npy"))
    assert outs[0].shape == (100,) and outs[0].max() < 200 and np.array_equal(outs[0], outs[1])
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, pix.size, 100, dtype=np.int64))
    assert np.array_equal(outs[0], pix[pos].astype(np.float32))
