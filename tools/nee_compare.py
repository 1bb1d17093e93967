#!/usr/bin/env python3
"""Next-event estimation beside the learned samplers: the default render (rt_render), NEE
(rt_render_nee), a radiance map Expected SARSA trained and a map baked from ground truth (both
rendered frozen), all at the same samples per pixel against a high-spp rt_render of the camera.

    python tools/nee_compare.py door_room [--size 256] [--spp 64] [--train 8] [--out-dir DIR]

One JSON line; per renderer
  mape8 / mape_f    rtmi.metrics against the reference frame (8-bit as Graphing/mape.py, and float)
  zero_share        zero-contribution paths / paths: NEE and the maps by their own counters, the
                    default render by the share of black pixels of --zero-frames one-sample frames
  casts_per_sample  ray casts / (pixels x spp), shadow casts included
  ms                the frame's wall time, best of --runs (tables and maps built before)
  equal_time_mse    the float frame's mean squared error x ms: what the error would be at equal
                    time, as the error of a Monte Carlo mean falls as 1 / samples
With --out-dir the four frames are written as PNGs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402


def load_scene(name):
    if name == "cornell":
        return rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
    return rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", name + ".obj"), name)


def best_of(fn, runs):
    best, res = None, None
    for _ in range(runs):
        t0 = time.perf_counter()
        res = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=sorted(rtmi.CAMERAS))
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--train", type=int, default=8, help="frames the trained map learns before it is frozen")
    ap.add_argument("--bake-spp", type=int, default=64)
    ap.add_argument("--zero-frames", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    S = rtmi.sarsa
    g = load_scene(args.scene)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    gp = lambda **kw: rtmi.default_params(rtmi.RT_PRESET_GPU, seed=args.seed, **kw)  # noqa: E731
    split = 8 if args.spp % 8 == 0 else 1
    p = gp(width=args.size, height=args.size, spp=args.spp, spp_split=split)
    samples = args.size * args.size * args.spp
    to8 = lambda x: rtmi.metrics.argb_to_rgb8(rtmi.pack_argb(x))  # noqa: E731
    out = {"scene": args.scene, "size": args.size, "spp": args.spp, "ref_spp": args.ref_spp, "train_frames": args.train,
           "bake_spp": args.bake_spp}
    frames = {}

    def row(name, ref, ms, img, casts, zero_share):
        mse = float(np.mean((img.astype(np.float64) - ref.astype(np.float64)) ** 2))
        frames[name] = img
        out[name] = {"mape8": rtmi.metrics.mape8(to8(ref), to8(img)), "mape_f": rtmi.metrics.mape_f(ref, img),
                     "mse": mse, "zero_share": zero_share, "casts_per_sample": casts / samples, "ms": round(ms, 2),
                     "equal_time_mse": mse * ms}

    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc:
        ref, _ = rtmi.render(ctx, sc, cam, gp(width=args.size, height=args.size, spp=args.ref_spp, spp_split=8))
        black = total = 0
        for k in range(args.zero_frames):
            one, _ = rtmi.render(ctx, sc, cam, rtmi.default_params(rtmi.RT_PRESET_GPU, width=args.size, height=args.size,
                                                                   spp=1, seed=args.seed + 1 + k))
            black += int((~one.any(axis=2)).sum())
            total += one.shape[0] * one.shape[1]
        ms, (img, casts) = best_of(lambda: rtmi.render(ctx, sc, cam, p), args.runs)
        row("default", ref, ms, img, casts, black / total)
        rtmi.render_nee(ctx, sc, cam, p, 0, rect=(0, 0, 16, 16))  # the tables
        ms, (img, casts, st) = best_of(lambda: rtmi.render_nee(ctx, sc, cam, p, 0, stats=True), args.runs)
        row("nee", ref, ms, img, casts, st["zero_paths"] / st["paths"])
        with S.RadianceMap(ctx, sc, args.seed) as rm:
            if args.train > 0:
                rm.render(cam, p, args.train)
            rm.set_td_mode(S.TD_OFF)
            ms, (img, casts) = best_of(lambda: rm.render(cam, p), args.runs)
            row("sarsa_trained", ref, ms, img, casts, rm.frame_stats()[1] / samples)
        with S.RadianceMap(ctx, sc, args.seed) as rm:
            rm.bake(sc, gp(spp=args.bake_spp, spp_split=4, t_scale=float(args.size)))
            rm.set_td_mode(S.TD_OFF)
            ms, (img, casts) = best_of(lambda: rm.render(cam, p), args.runs)
            row("sarsa_baked", ref, ms, img, casts, rm.frame_stats()[1] / samples)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        for name, img in frames.items():
            rtmi.save_png(os.path.join(args.out_dir, f"{args.scene}_{name}.png"), rtmi.pack_argb(img))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
