#!/usr/bin/env python3
"""The thesis's two-panel figure fig:direct_and_global
(Descriptions/write_up/chapters/1_conceptual_background.tex:24-38): a scene lit by direct light
alone beside the same scene with global illumination, at equal samples per pixel.

    python tools/direct_and_global.py cornell [--size 512] [--spp 64] [--out-dir .]

Writes <scene>_direct.png (rt_render_nee with RT_NEE_DIRECT_ONLY: the first surface's direct
light), <scene>_global.png (rt_render_nee, flags 0) and <scene>_direct_and_global.png (the two
side by side), and prints one JSON line with the files, the casts and the frame times.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=sorted(rtmi.CAMERAS))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--out-dir", default=".")
    args = ap.parse_args()
    g = load_scene(args.scene)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=args.size, height=args.size, spp=args.spp, seed=args.seed,
                            spp_split=8 if args.spp % 8 == 0 else 1)
    os.makedirs(args.out_dir, exist_ok=True)
    out = {"scene": args.scene, "size": args.size, "spp": args.spp}
    frames = {}
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc:
        rtmi.render_nee(ctx, sc, cam, p, 0, rect=(0, 0, 16, 16))  # the candidate table and the light table
        for name, flags in (("direct", rtmi.RT_NEE_DIRECT_ONLY), ("global", 0)):
            t0 = time.perf_counter()
            img, casts, st = rtmi.render_nee(ctx, sc, cam, p, flags, stats=True)
            ms = (time.perf_counter() - t0) * 1e3
            frames[name] = rtmi.pack_argb(img)
            path = os.path.join(args.out_dir, f"{args.scene}_{name}.png")
            rtmi.save_png(path, frames[name])
            out[name] = {"file": path, "casts": casts, "ms": round(ms, 2), "zero_share": st["zero_paths"] / st["paths"]}
    both = os.path.join(args.out_dir, f"{args.scene}_direct_and_global.png")
    rtmi.save_png(both, np.concatenate([frames["direct"], frames["global"]], axis=1))
    out["figure"] = both
    print(json.dumps(out))


if __name__ == "__main__":
    main()
