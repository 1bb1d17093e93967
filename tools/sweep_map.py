#!/usr/bin/env python3
"""Value iteration over the radiance map: expected-value sweeps (rt_sarsa_sweep) from a fresh map,
how fast the irradiance estimates settle, and what the swept map is worth as a sampler beside a
fresh map, a map trained by frames and a map baked from ground truth.

    python tools/sweep_map.py [door_room] [--replace 8] [--mean 4] [--spp 8] [--render-spp 128]

One JSON line per sweep ("sweep": its index, "replace": whether the map forgot first, the largest
and the median absolute change of the volumes' irradiance estimates, the same relative to the
largest estimate, k_sweep's milliseconds (rt_ktime) and casts, and the mean squared error of
--curve-frames frozen frames of --curve-spp at --curve-size^2 against the reference, their mean and
their largest: the curve the tests' sweep count is read from), then one line with
  mape8 / mape_f / mse   of the --render-spp frozen render at --size^2 against rt_render at --ref-spp
                         for "fresh", "trained" (--train frames of --render-spp), "baked" (--bake-spp
                         paths per sector) and "swept"
  tv_median              the median over the volumes of the total variation of the normalised Q rows
                         from the baked map's, for fresh, trained and swept
  ms                     k_bake's, the training frames' k_sarsa_render and the sweeps' k_sweep milliseconds
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402

from bake_map import errors, ktime_of, load_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", nargs="?", default="door_room", choices=sorted(rtmi.CAMERAS))
    ap.add_argument("--area", type=float, default=None, help="AREA_PER_SAMPLE (default: the reference's 0.001)")
    ap.add_argument("--replace", type=int, default=8, help="replace sweeps (forget first)")
    ap.add_argument("--mean", type=int, default=4, help="mean sweeps after them")
    ap.add_argument("--spp", type=int, default=8, help="casts per sector and sweep")
    ap.add_argument("--render-spp", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--curve-size", type=int, default=64)
    ap.add_argument("--curve-spp", type=int, default=16)
    ap.add_argument("--curve-frames", type=int, default=8)
    ap.add_argument("--train", type=int, default=8)
    ap.add_argument("--bake-spp", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1984)
    args = ap.parse_args()
    S = rtmi.sarsa
    g = load_scene(args.scene)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    gp = lambda **kw: rtmi.default_params(rtmi.RT_PRESET_GPU, seed=args.seed, **kw)  # noqa: E731
    split = lambda n: 8 if n % 8 == 0 else 1  # noqa: E731
    p = gp(width=args.size, height=args.size, spp=args.render_spp, spp_split=split(args.render_spp))
    pc = gp(width=args.curve_size, height=args.curve_size, spp=args.curve_spp, spp_split=split(args.curve_spp))
    ps = gp(spp=args.spp, t_scale=float(args.size))
    pb = gp(spp=args.bake_spp, spp_split=4 if args.bake_spp % 4 == 0 else 1, t_scale=float(args.size))
    tv = lambda qt, q: float(np.nanmedian(rtmi.probe.distribution_error(qt, q)["tv"]))  # noqa: E731
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc:
        new_map = lambda: S.RadianceMap(ctx, sc, args.seed, args.area)  # noqa: E731
        ref, _ = rtmi.render(ctx, sc, cam, gp(width=args.size, height=args.size, spp=args.ref_spp, spp_split=8))
        refc, _ = rtmi.render(ctx, sc, cam, gp(width=args.curve_size, height=args.curve_size, spp=args.ref_spp,
                                               spp_split=8))

        def frozen(rm, params, reference):
            rm.set_td_mode(S.TD_OFF)
            e = errors(reference, rm.render(cam, params)[0])
            rm.set_td_mode(S.TD_FRAME)
            return e

        def curve(rm):
            e = [frozen(rm, pc, refc)["mse"] for _ in range(args.curve_frames)]
            return {"curve_mse": float(np.mean(e)), "curve_mse_max": float(np.max(e))}

        out = {"scene": args.scene, "size": args.size, "render_spp": args.render_spp, "ref_spp": args.ref_spp,
               "sweep_spp": args.spp, "replace": args.replace, "mean": args.mean, "ms": {}}
        with new_map() as rm:
            out["volumes"] = rm.n_volumes
            q_fresh = rm.read()[0]
            out["fresh"] = frozen(rm, p, ref)
        with new_map() as rm:
            out["ms"]["train_frames"] = [ktime_of(rtmi.RT_KT_SARSA_RENDER, lambda: rm.render(cam, p))[0]
                                         for _ in range(args.train)]
            q_trained = rm.read()[0]
            out["trained"] = frozen(rm, p, ref)
        with new_map() as rm:
            out["ms"]["k_bake"] = ktime_of(rtmi.RT_KT_BAKE, lambda: rm.bake(sc, pb))[0]
            q_baked = rm.read()[0]
            out["baked"] = frozen(rm, p, ref)
        with new_map() as rm:
            irr = rm.read()[3]
            print(json.dumps({"sweep": -1, **curve(rm)}), flush=True)
            sweep_ms = []
            for k in range(args.replace + args.mean):
                replace = k < args.replace
                if replace:
                    rm.forget()
                ms, casts = ktime_of(rtmi.RT_KT_BAKE, lambda: rm.sweep(sc, ps, first_sample=k * args.spp))
                sweep_ms.append(ms)
                now = rm.read()[3]
                d = np.abs(now.astype(np.float64) - irr)
                top = float(np.abs(now).max())
                print(json.dumps({"sweep": k, "replace": replace, "irr_change_max": float(d.max()),
                                  "irr_change_median": float(np.median(d)), "irr_change_max_rel": float(d.max()) / top,
                                  "irr_change_median_rel": float(np.median(d)) / top, "k_sweep_ms": ms, "casts": casts,
                                  **curve(rm)}), flush=True)
                irr = now
            out["ms"]["k_sweep"] = sweep_ms
            out["swept"] = frozen(rm, p, ref)
            out["tv_median"] = {"fresh": tv(q_baked, q_fresh), "trained": tv(q_baked, q_trained),
                                "swept": tv(q_baked, rm.read()[0])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
