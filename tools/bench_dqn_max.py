#!/usr/bin/env python3
"""One DQN frame in the three ways the renderer can sample it, beside each other.

    python tools/bench_dqn_max.py [--scene archway] [--width 1024] [--spp 16] [--rounds 7] [--out FILE]

One process, one network (the benchmark's synthetic weights unless --model names a DyNet file):
rt_render_dqn_tiles_device in RT_DQN_SAMPLE_CDF, in RT_DQN_SAMPLE_MAX with the action taken in the
forward's epilogue (RTMI_DQN_MAX_FUSED=1), and in RT_DQN_SAMPLE_MAX with the forward writing
fp32 Q and k_dqn_argmax reading it back (RTMI_DQN_MAX_FUSED=0).  Every variant is warmed up with
one frame, then --rounds rounds alternate the variants; a timing is one whole frame between two
device events on the stream (the render synchronises the stream itself every few bounces, so the
events bracket finished work).  Reported per variant: median, minimum and maximum of the rounds,
ray casts and zero-contribution paths of the frame (rt_dqn_render_stats); the two max-mode
routes' images are compared bit for bit at the timed size.  A max-mode frame casts a different
number of rays than a CDF frame, so ms per frame and ns per cast are both given.  Prints one JSON
line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="archway")
    ap.add_argument("--model", default=None, help="DyNet model (default: synthetic_weights, as bench.py)")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tile", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_max", "bench_dqn_max.json"))
    args = ap.parse_args()
    W = H = args.width
    dev = torch.device("cuda", 0)
    g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", args.scene + ".obj"), args.scene)
    if args.model:
        Wt, b = rtmi.dqn.split_layers(rtmi.dqn.read_dynet(args.model))
    else:
        Wt, b = rtmi.dqn.synthetic_weights(g.nn_vertices.size, seed=args.seed)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=W, height=H, spp=args.spp, spp_split=1, seed=args.seed)
    variants = ("cdf", "max_fused", "max_written_out")
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc, rtmi.dqn.Dqn(ctx, g.nn_vertices, Wt, b) as net:
        origins = rtmi.tiles.tile_origins(W, H, args.tile)
        out = torch.zeros((len(origins), args.tile, args.tile, 3), dtype=torch.float32, device=dev)
        casts = torch.zeros(1, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream()

        def timed(v):
            net.set_sampling(net.SAMPLE_CDF if v == "cdf" else net.SAMPLE_MAX)
            os.environ["RTMI_DQN_MAX_FUSED"] = "0" if v == "max_written_out" else "1"
            casts.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rtmi.dqn.render_tiles_device(ctx, sc, net, cam, p, origins, args.tile, out.data_ptr(), casts.data_ptr(),
                                         stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        images, frame = {}, {}
        rtmi.dqn.enable_stats(ctx, True)   # (the warm-up frames count; the timed ones do not)
        for v in variants:  # warm-up, and the images and counts of the timed size
            timed(v)
            images[v] = out.cpu().numpy().copy()
            paths, zero = rtmi.dqn.render_stats(ctx)
            frame[v] = {"casts": int(casts.item()), "paths": paths, "zero_paths": zero}
        same = bool(np.array_equal(images["max_fused"].view(np.uint32), images["max_written_out"].view(np.uint32)))
        rtmi.dqn.enable_stats(ctx, False)
        ms = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v in variants:
                ms[v].append(timed(v))
        net.set_sampling(net.SAMPLE_CDF)
        med = {v: statistics.median(ms[v]) for v in variants}
        result = {
            "scene": args.scene, "model": os.path.basename(args.model) if args.model else "synthetic_weights",
            "width": W, "height": H, "spp": args.spp, "max_bounces": p.max_bounces, "rounds": args.rounds,
            "max_fused_equals_written_out_bits": same,
            "variants": {v: {"ms_median": med[v], "ms_min_max": [min(ms[v]), max(ms[v])],
                             "ns_per_cast": 1e6 * med[v] / max(frame[v]["casts"], 1),
                             "mean_path_length": frame[v]["casts"] / frame[v]["paths"],
                             "zero_path_share": frame[v]["zero_paths"] / frame[v]["paths"], **frame[v]}
                         for v in variants},
            "fused_over_written_out": med["max_fused"] / med["max_written_out"],
            "written_out_spread_ms": max(ms["max_written_out"]) - min(ms["max_written_out"]),
        }
    os.environ.pop("RTMI_DQN_MAX_FUSED", None)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
