#!/usr/bin/env python
"""What the output formats cost: python tools/format_bench.py [--batch 256] [--rounds 3] > profiles/NAME.json

Workload: a fixed seeded batch of 1920x1080 4:2:0 q90 images with DRI = one MCU row
(jd_synth.make_batch), inputs and outputs resident in HBM.  For each of the five output formats
(interleaved RGB, interleaved BGR, planar RGB, planar BGR, gray), one Decoder each, in one process:

  * step_ms: the pipelined step on the context's own streams, 5 warm-up and 20 timed steps bracketed
    by a device synchronise, as bench.py times its flagship;
  * idct_ms: k_idct_color's time per launch, from a separate serialized pass (JD_FLAG_TIMING's
    hipEvents around every kernel).

And what a caller who wants CHW does without the planar format, next to the planar decode, both
ordered on one torch stream (hip_stream) so that the permute runs behind the decode it reads:

  * stream_chw_ms: the planar decode;
  * stream_rgb_ms: the default decode;
  * stream_rgb_permute_ms: the default decode followed by permute(0, 3, 1, 2).contiguous() over the
    batch's [N, H, W, 3] tensor.

The variants alternate within each of --rounds rounds, so every figure comes as one value per round
with its median and spread (max - min).  Image 0 of every format is checked against the oracle first.
One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before jdamd loads libjdamd.so (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gpu-jpeg-decoder_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import jd_synth  # noqa: E402
import jdamd  # noqa: E402
import jdoracle  # noqa: E402

FORMATS = {"rgb": ("hwc", "rgb"), "bgr": ("hwc", "bgr"), "chw": ("chw", "rgb"), "chw-bgr": ("chw", "bgr"),
           "gray": ("hwc", "gray")}
W, H = 1920, 1080


def summary(xs):
    return {"rounds": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4),
            "spread": round(max(xs) - min(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-steps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.batch
    datas = jd_synth.make_batch(n, W, H, 90, "4:2:0", 1, 0, seed0=424242, workers=min(16, os.cpu_count() or 1))
    hosts = [np.frombuffer(x, np.uint8).copy() for x in datas]
    in_offs, tot = [], 0
    for h in hosts:
        in_offs.append(tot)
        tot += (h.nbytes + 64 + 255) // 256 * 256
    flat = np.zeros(tot, np.uint8)
    for h, o in zip(hosts, in_offs):
        flat[o:o + h.nbytes] = h
    jpeg_dev = torch.from_numpy(flat).to(dev)
    img3 = W * H * 3  # a multiple of 256: the batch's outputs are one dense [N, H, W, 3] / [N, 3, H, W] tensor
    bufs = [torch.empty(n * img3, dtype=torch.uint8, device=dev) for _ in range(3)]
    side = torch.cuda.Stream(dev)

    decs, batches = {}, {}
    for name, (layout, channels) in FORMATS.items():
        dec = jdamd.Decoder(0, timing=True, layout=layout, channels=channels)
        per = W * H * (1 if channels == "gray" else 3)
        decs[name] = dec
        batches[name] = [dec.make_batch(hosts, [jpeg_dev.data_ptr() + o for o in in_offs],
                                        [b.data_ptr() + i * per for i in range(n)]) for b in bufs]
        # image 0 against the oracle, once
        dec.decode_prepared(batches[name][0])
        assert not any(r.status for r in batches[name][0][1]), name
        got = bufs[0][:per].cpu().numpy().reshape(dec.output_shape(H, W))
        st, ref = jdoracle.decode(datas[0])
        assert st == 0
        if channels != "gray":
            ref = ref[..., ::-1] if channels == "bgr" else ref
            ref = ref.transpose(2, 0, 1) if layout == "chw" else ref
            assert np.array_equal(got, ref), name
        else:
            assert got.shape == (H, W)

    def timed(name, stream=None, permute=False):
        dec, bt = decs[name], batches[name]
        hs = stream.cuda_stream if stream is not None else None
        keep = None

        def step(k):
            nonlocal keep
            dec.decode_prepared(bt[k % 3], stream=hs, pipelined=True)
            if permute:  # behind the decode on the same stream
                with torch.cuda.stream(stream):
                    keep = bufs[k % 3].view(n, H, W, 3).permute(0, 3, 1, 2).contiguous()

        for k in range(max(3, args.warmup)):
            step(k)
        dec.wait()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for k in range(args.steps):
            step(k)
        dec.wait()
        torch.cuda.synchronize(dev)
        del keep
        return (time.perf_counter() - t0) / args.steps * 1e3

    def idct_ms(name):
        dec, bt = decs[name], batches[name]
        dec.decode_prepared(bt[0])
        dec.reset_stats()
        for k in range(args.kernel_steps):
            dec.decode_prepared(bt[k % 3])
        k = dec.stats()["kernels"]["k_idct_color"]
        return k["total_ms"] / k["launches"]

    step = {f: [] for f in FORMATS}
    idct = {f: [] for f in FORMATS}
    on_stream = {"stream_chw_ms": [], "stream_rgb_ms": [], "stream_rgb_permute_ms": []}
    for _ in range(args.rounds):
        for f in FORMATS:
            step[f].append(timed(f))
        for f in FORMATS:
            idct[f].append(idct_ms(f))
        on_stream["stream_chw_ms"].append(timed("chw", side))
        on_stream["stream_rgb_ms"].append(timed("rgb", side))
        on_stream["stream_rgb_permute_ms"].append(timed("rgb", side, permute=True))
    for dec in decs.values():
        dec.close()
    out = {"metric": "output formats: pipelined step and k_idct_color per launch (ms)",
           "workload": f"{n} x {W}x{H} 4:2:0 q90, DRI = 1 MCU row, seed0 424242, inputs and outputs in HBM",
           "steps": args.steps, "warmup": args.warmup, "kernel_steps": args.kernel_steps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(dev),
           "step_ms": {f: summary(v) for f, v in step.items()},
           "idct_ms": {f: summary(v) for f, v in idct.items()}}
    out.update({k: summary(v) for k, v in on_stream.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
