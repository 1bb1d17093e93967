#!/usr/bin/env python3
"""The ground-truth probe's rate beside the GPU-preset render's, same scene, same process.

    python tools/bench_probe.py [--scenes cornell,complex_light_room] [--points 4096] [--spp 16] [--split 4]

Per scene: rt_probe_radiance on one batch of points large enough to fill the device (the
positions and surfaces of radiance volumes spread evenly over the scene's map; points x 144 x
spp paths in points x 144 x split queue items -- several per lane of the persistent grid: at 1.5
items per lane, 4096 points unsplit, a quarter of the lanes idle through the second round),
k_probe timed by rt_ktime (a warm-up call, which also builds the candidate table,
then the median of --runs calls), and next to it rt_render's GPU preset on the scene's own camera
(k_render_pq, the same casts through the same table and exact phase), timed the same way.
Reported: paths/s and casts/s of the probe, casts/s of the render, and their ratio -- a figure,
not a gate.  One JSON line per scene.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402


def ktime_of(fam, fn):
    rtmi.ktime_enable(True)
    out = fn()
    ms, n = rtmi.ktime_read()[fam]
    rtmi.ktime_enable(False)
    return ms, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell,complex_light_room")
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--spp", type=int, default=16, help="paths per sector")
    ap.add_argument("--split", type=int, default=4, help="spp_split: chunks per sector (queue items)")
    ap.add_argument("--render-width", type=int, default=1024)
    ap.add_argument("--render-spp", type=int, default=32)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--probe-only", action="store_true", help="skip the render (counter runs of k_probe)")
    args = ap.parse_args()
    med = statistics.median
    for name in args.scenes.split(","):
        if name == "cornell":
            g = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
        else:
            g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", name + ".obj"), name)
        with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc:
            with rtmi.sarsa.RadianceMap(ctx, sc, 1984) as rm:
                vpos, _, vsurf, _ = rm.volumes()
            idx = np.unique(np.linspace(0, len(vpos) - 1, min(args.points, len(vpos))).astype(np.int64))
            pos, tri, ids = vpos[idx], vsurf[idx], idx.astype(np.uint32)
            p = rtmi.default_params(rtmi.RT_PRESET_GPU, spp=args.spp, spp_split=args.split)

            def probe():
                return rtmi.probe.radiance(ctx, sc, p, pos, tri, ids, want_irr=True)

            probe()  # warm-up
            ms, casts = [], 0
            for _ in range(args.runs):
                t, got = ktime_of(rtmi.RT_KT_PROBE, probe)
                ms.append(t)
                casts = got["casts"]
            paths = len(idx) * rtmi.probe.SECTORS * args.spp
            line = {"scene": name, "triangles": g.n_tri, "points": int(len(idx)), "spp": args.spp, "spp_split": args.split,
                    "max_bounces": p.max_bounces, "paths": paths, "casts": casts, "casts_per_path": casts / paths,
                    "probe_kernel_ms": med(ms), "probe_kernel_ms_min_max": [min(ms), max(ms)],
                    "probe_paths_per_s": paths / (med(ms) * 1e-3), "probe_casts_per_s": casts / (med(ms) * 1e-3),
                    "ctab_built": sc.ctab_info(p.hit_rule)["built"]}
            if not args.probe_only:
                W = args.render_width
                pr = rtmi.default_params(rtmi.RT_PRESET_GPU, width=W, height=W, spp=args.render_spp, spp_split=1)
                cam = rtmi.camera(rtmi.CAMERAS[name])

                def render():
                    return rtmi.render(ctx, sc, cam, pr)[1]

                render()
                rms, rcasts = [], 0
                for _ in range(args.runs):
                    t, rcasts = ktime_of(rtmi.RT_KT_RENDER, render)
                    rms.append(t)
                line.update({"render": f"{W}x{W}x{args.render_spp}", "render_casts": rcasts,
                             "render_casts_per_path": rcasts / (W * W * args.render_spp),
                             "render_kernel_ms": med(rms), "render_casts_per_s": rcasts / (med(rms) * 1e-3),
                             "probe_over_render_casts_per_s": (casts / med(ms)) / (rcasts / med(rms))})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
