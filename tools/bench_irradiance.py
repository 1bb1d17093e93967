#!/usr/bin/env python3
"""The irradiance render (k_sarsa_irr) beside the radiance-map view (k_sarsa_view) of the same map
and frame: the same camera casts, a k-nearest search instead of the single-nearest one.

    python tools/bench_irradiance.py [--scenes door_room cornell] [--width 720] [--spp 16] [--rounds 9]

Per scene, in one process: the map is baked at --bake-spp, every variant is warmed up, then
--rounds rounds alternate the variants; each timing is --reps launches over the whole image
(rt_render_irradiance_tiles_device / rt_render_volume_view_tiles_device into device memory)
between two device events on the stream.  Variants: the view, and the irradiance render at
(k = 1, mean), (k = 3, mean), (k = 8, mean), (k = 8, cone), all at the map's reach.  Reports per
variant the median and range of the milliseconds per launch, the ratio of the medians to the
view's, and search queries (surface-hit samples) per second.  Prints one JSON line.
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
    ap.add_argument("--scenes", nargs="+", default=["door_room", "cornell"])
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--split", type=int, default=16, help="spp_split: lanes per pixel (the view's fastest is spp)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20, help="launches per timing")
    ap.add_argument("--bake-spp", type=int, default=4)
    ap.add_argument("--tile", type=int, default=240)
    ap.add_argument("--seed", type=int, default=1984)
    args = ap.parse_args()
    W = H = args.width
    S = rtmi.sarsa
    dev = torch.device("cuda", 0)
    variants = [("view", None), ("k1_mean", (1, rtmi.RT_IRR_MEAN)), ("k3_mean", (3, rtmi.RT_IRR_MEAN)),
                ("k8_mean", (8, rtmi.RT_IRR_MEAN)), ("k8_cone", (8, rtmi.RT_IRR_CONE))]
    result = {"width": W, "height": H, "spp": args.spp, "spp_split": args.split, "rounds": args.rounds,
              "reps": args.reps, "bake_spp": args.bake_spp, "scenes": {}}
    for scene in args.scenes:
        if scene == "cornell":
            g = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
        else:
            g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", scene + ".obj"), scene)
        cam = rtmi.camera(rtmi.CAMERAS[scene])
        p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=W, height=H, spp=args.spp, spp_split=args.split,
                                seed=args.seed)
        p1 = rtmi.default_params(rtmi.RT_PRESET_GPU, width=W, height=H, spp=1, seed=args.seed)
        pb = rtmi.default_params(rtmi.RT_PRESET_GPU, spp=args.bake_spp, spp_split=1, t_scale=float(H), seed=args.seed)
        with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc, S.RadianceMap(ctx, sc, args.seed) as rm:
            rm.bake(sc, pb)
            rm.set_view_colours(S.irradiance_colours(rm.read()[3]))
            origins = rtmi.tiles.tile_origins(W, H, args.tile)
            out = torch.zeros((len(origins), args.tile, args.tile, 3), dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream()
            # the searches of one launch: the surface-hit samples, and what they find at k = 8
            queries, found = 0, np.zeros(9, np.int64)
            for s in range(args.spp):
                _, tri, _, vol, _ = rm.irradiance_view(cam, p1, 8, None, first_sample=s, aov=True)
                surf = (tri >= 0) & (tri < g.n_surf)
                queries += int(surf.sum())
                found += np.bincount((vol[surf] >= 0).sum(axis=1), minlength=9)

            def launch(v):
                if v is None:
                    rm.view_tiles_device(cam, p, origins, args.tile, out.data_ptr(), stream.cuda_stream)
                else:
                    rm.irradiance_view_tiles_device(cam, p, origins, args.tile, out.data_ptr(), stream.cuda_stream,
                                                    k=v[0], weight=v[1])

            def timed(v):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.reps):
                    launch(v)
                e1.record(stream)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / args.reps

            for _, v in variants:  # warm-up
                timed(v)
            ms = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, v in variants:
                    ms[name].append(timed(v))
            med = {name: statistics.median(t) for name, t in ms.items()}
            result["scenes"][scene] = {
                "volumes": rm.n_volumes, "reach": rm.knn_reach(), "queries_per_launch": queries,
                "found_at_k8_histogram": found.tolist(),
                "variants": {name: {"ms_median": med[name], "ms_min_max": [min(ms[name]), max(ms[name])],
                                    "ratio_to_view": med[name] / med["view"],
                                    "queries_per_s": queries / (med[name] * 1e-3)} for name, _ in variants},
            }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
