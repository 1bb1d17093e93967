#!/usr/bin/env python3
"""The bench frame with a camera that moves every frame.

bench.py renders one view over and over, so the primary-ray cull's forms (k_cull_forms) are
computed once.  Here two cameras alternate frame by frame: the forms kernel runs ahead of every
k_render_ps launch, which is what a moving camera pays.  Same frame as bench.py's default line
(Cornell box, CPU preset, 512^2 x 256 spp, spp_split 64); compare builds with RTMI_LIB, each
run a process of its own.

    python tools/bench_moving_camera.py [--steps 40] [--warmup 4] [--still]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--still", action="store_true", help="one camera only (bench.py's case)")
    args = ap.parse_args()
    geom = rtmi.cornell_geometry(rtmi.RT_PRESET_CPU)
    p = rtmi.default_params(rtmi.RT_PRESET_CPU, width=512, height=512, spp=256, spp_split=64)
    pos = rtmi.CAMERAS["cornell"]
    cams = [rtmi.camera(pos), rtmi.camera((pos[0] + 0.05, pos[1], pos[2], pos[3]), yaw_y=0.02)]
    if args.still:
        cams = cams[:1]
    tiles = rtmi.tiles.rank_tiles(512, 512, 32, 0, 1)
    stream = torch.cuda.current_stream()
    out = torch.zeros((len(tiles), 32, 32, 3), device="cuda")
    casts = torch.zeros(1, dtype=torch.int64, device="cuda")
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, geom) as sc:
        def frame(i):
            rtmi.render_tiles_device(ctx, sc, cams[i % len(cams)], p, tiles, 32, out.data_ptr(), casts.data_ptr(),
                                     stream.cuda_stream)
        for i in range(args.warmup):
            frame(i)
        torch.cuda.synchronize()
        casts.zero_()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        t0 = time.perf_counter()
        for i in range(args.steps):
            ev[i][0].record(stream)
            frame(i)
            ev[i][1].record(stream)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    ms = [a.elapsed_time(b) for a, b in ev]
    print(json.dumps({"cameras": len(cams), "steps": args.steps, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
                      "event_ms_median": round(float(np.median(ms)), 4), "event_ms_min": round(min(ms), 4),
                      "ray_casts": int(casts.item()), "image_sum": float(out.double().sum().item()),
                      "lib": os.path.relpath(rtmi._lib.LIB_PATH, ROOT)}))


if __name__ == "__main__":
    main()
