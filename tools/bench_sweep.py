#!/usr/bin/env python3
"""k_sweep beside k_bake at max_bounces = 2: that bake casts the same first rays of every (volume,
sector, sample) and neither searches the map nor deposits, so the ratio of the two kernel times is
the cost of the nearest-volume search plus the deposit.

    python tools/bench_sweep.py [door_room] [--spp 1 4 16] [--runs 3]

One JSON line: per spp the casts, the fastest of --runs kernel times (rt_ktime, milliseconds) and
casts/s of k_sweep (apply = 0: the kernel alone; the pending sums grow, which costs nothing) and
of k_bake, and their ratio; k_sarsa_apply's milliseconds after a sweep; and, for scale, one
training frame (k_sarsa_render at --frame-size^2 x --frame-spp) of the same map.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402

from bake_map import ktime_of, load_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", nargs="?", default="door_room", choices=sorted(rtmi.CAMERAS))
    ap.add_argument("--area", type=float, default=None, help="AREA_PER_SAMPLE (default: the reference's 0.001)")
    ap.add_argument("--spp", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--t-scale", type=float, default=256.0)
    ap.add_argument("--frame-size", type=int, default=512)
    ap.add_argument("--frame-spp", type=int, default=256)
    ap.add_argument("--seed", type=int, default=1984)
    args = ap.parse_args()
    S = rtmi.sarsa
    g = load_scene(args.scene)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    gp = lambda **kw: rtmi.default_params(rtmi.RT_PRESET_GPU, seed=args.seed, t_scale=args.t_scale, **kw)  # noqa: E731
    out = {"scene": args.scene, "t_scale": args.t_scale, "runs": args.runs, "spp": {}}
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc:
        with S.RadianceMap(ctx, sc, args.seed, args.area) as sw, S.RadianceMap(ctx, sc, args.seed, args.area) as bk:
            out["volumes"] = sw.n_volumes
            sw.sweep(sc, gp(spp=1), apply=False)  # warm-up: the scene's candidate table
            for spp in args.spp:
                ps, pb = gp(spp=spp), gp(spp=spp, spp_split=1, max_bounces=2)
                s_ms, b_ms, casts, b_casts = [], [], 0, 0
                for _ in range(args.runs):
                    ms, casts = ktime_of(rtmi.RT_KT_BAKE, lambda: sw.sweep(sc, ps, apply=False))
                    s_ms.append(ms)
                    ms, b_casts = ktime_of(rtmi.RT_KT_BAKE, lambda: bk.bake(sc, pb))
                    b_ms.append(ms)
                assert casts == b_casts == sw.n_volumes * S.SECTORS * spp
                out["spp"][str(spp)] = {"casts": casts, "k_sweep_ms": s_ms, "k_bake_ms": b_ms,
                                        "k_sweep_casts_per_s": casts / (min(s_ms) * 1e-3),
                                        "k_bake_casts_per_s": casts / (min(b_ms) * 1e-3),
                                        "sweep_over_bake": min(s_ms) / min(b_ms)}
            out["k_sarsa_apply_ms"] = ktime_of(rtmi.RT_KT_SARSA_APPLY, lambda: sw.apply())[0]
            pf = gp(width=args.frame_size, height=args.frame_size, spp=args.frame_spp, spp_split=8)
            pf.t_scale = float(args.frame_size)
            sw.render(cam, pf)  # warm-up
            out["frame"] = {"size": args.frame_size, "spp": args.frame_spp,
                            "k_sarsa_render_ms": [ktime_of(rtmi.RT_KT_SARSA_RENDER, lambda: sw.render(cam, pf))[0]
                                                  for _ in range(args.runs)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
