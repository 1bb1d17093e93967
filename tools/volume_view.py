#!/usr/bin/env python3
"""Radiance-map views of a scene as PNGs: what each camera hit's nearest radiance volume is
(the reference's Voronoi view, GPU/main.cu PATH_TRACING_METHOD 2) and what the map has learned.

    python tools/volume_view.py door_room [--train N] [--width 720] [--spp 4] [--irradiance K] [--out DIR]

Optionally trains N Expected-SARSA frames first, then writes
    <scene>_voronoi.png     the random per-volume palette of the map's seed
    <scene>_irradiance.png  each volume's irradiance estimate as grey
    <scene>_visits.png      each volume's visits, log scale
    <scene>_max_q.png       the sector of largest Q as hue / value
and with --irradiance K
    <scene>_irradiance_k<K>.png  the irradiance render (rt_render_irradiance): each hit as the mean
                            estimate of its K nearest volumes times the surface's colour, lights lit
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=sorted(rtmi.CAMERAS))
    ap.add_argument("--train", type=int, default=0, help="Expected-SARSA frames rendered before the views")
    ap.add_argument("--train-spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--spp", type=int, default=4, help="samples per pixel of the views")
    ap.add_argument("--irradiance", type=int, default=0, metavar="K",
                    help="also the irradiance render interpolated over the K nearest volumes (1..8)")
    ap.add_argument("--area-per-sample", type=float, default=None, help="volume density (default 0.001)")
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    w, h = args.width, args.height or args.width
    if args.scene == "cornell":
        g = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
    else:
        g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", args.scene + ".obj"), args.scene)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    os.makedirs(args.out, exist_ok=True)
    S = rtmi.sarsa
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc, \
            S.RadianceMap(ctx, sc, args.seed, args.area_per_sample) as rm:
        print(f"{args.scene}: {rm.n_volumes} radiance volumes")
        if args.train > 0:
            pt = rtmi.default_params(rtmi.RT_PRESET_GPU, width=w, height=h, spp=args.train_spp)
            rm.render(cam, pt, args.train)
            print(f"trained {args.train} frames of {args.train_spp} spp")
        q, _, visits, irradiance = rm.read()
        # one lane per sample where spp allows it: the view's fastest layout
        split = args.spp if args.spp <= 64 and args.spp & (args.spp - 1) == 0 else 1
        p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=w, height=h, spp=args.spp, spp_split=split)
        tables = (("voronoi", None), ("irradiance", S.irradiance_colours(irradiance)),
                  ("visits", S.visits_colours(visits)), ("max_q", S.max_q_colours(q)))
        for name, table in tables:
            rm.set_view_colours(table)
            path = os.path.join(args.out, f"{args.scene}_{name}.png")
            rtmi.save_png(path, rtmi.pack_argb(rm.view(cam, p)))
            print("wrote", path)
        if args.irradiance > 0:
            path = os.path.join(args.out, f"{args.scene}_irradiance_k{args.irradiance}.png")
            rtmi.save_png(path, rtmi.pack_argb(rm.irradiance_view(cam, p, args.irradiance)))
            print("wrote", path)


if __name__ == "__main__":
    main()
