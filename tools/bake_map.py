#!/usr/bin/env python3
"""How good can importance sampling from the 12 x 12 radiance map get: the map filled from ground
truth (rt_sarsa_bake) and rendered frozen (RT_SARSA_TD_OFF), beside the default render and a map
that Expected SARSA trained, all at the same samples per pixel against a high-spp rt_render of
the same camera.

    python tools/bake_map.py door_room [--spp 64] [--render-spp 128] [--train 8] [--frame-time]

One JSON line:
  mape8 / mape_f   rtmi.metrics of (a) "default": rt_render, (b) "trained": a map trained --train
                   frames of --render-spp and then rendered frozen, (c) "baked": a fresh map baked
                   at --spp paths per sector and rendered frozen; mape8 on the packed 8-bit frames
                   (the reference's Graphing/mape.py), mape_f on the float frames
  irradiance       the same errors of the one-sample irradiance render of the baked map
                   (rt_render_irradiance: no bounce, the map's own estimate at each camera hit) for
                   (k = 1, mean), (k = 3, mean) and (k = 8, cone) at the map's reach
  bake             volumes, paths, casts, the wall seconds of each of --runs bakes of the whole map
                   (the first builds the scene's candidate table), k_bake's own milliseconds
                   (rt_ktime), paths/s and casts/s of the fastest
  map_tv           quantiles over the map of the total variation between the baked map's
                   normalised Q and an independent probe (first_sample past the bake's samples),
                   and the same for the trained map
  frame_ms         with --frame-time: k_sarsa_render's milliseconds (rt_ktime) of frames of the
                   baked map at --frame-size^2 x --frame-spp in RT_SARSA_TD_OFF and in
                   RT_SARSA_TD_FRAME, alternating, --runs each
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

QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)


def load_scene(name):
    if name == "cornell":
        return rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
    return rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", name + ".obj"), name)


def errors(ref, img):
    to8 = lambda x: rtmi.metrics.argb_to_rgb8(rtmi.pack_argb(x))  # noqa: E731
    return {"mape8": rtmi.metrics.mape8(to8(ref), to8(img)), "mape_f": rtmi.metrics.mape_f(ref, img),
            "mse": float(np.mean((img.astype(np.float64) - ref.astype(np.float64)) ** 2))}


def map_tv(ctx, sc, rm, p, first, batch=4096):
    """TV of the map's normalised Q against a probe of every volume at samples first .. first + spp"""
    pos, _, surf, _ = rm.volumes()
    q = rm.read()[0]
    tv = []
    for b in range(0, rm.n_volumes, batch):
        idx = np.arange(b, min(b + batch, rm.n_volumes))
        got = rtmi.probe.radiance(ctx, sc, p, pos[idx], surf[idx], idx, first, want_irr=False)
        tv.append(rtmi.probe.distribution_error(rtmi.probe.distribution(got["rad"]), q[idx])["tv"])
    tv = np.concatenate(tv)
    fin = tv[np.isfinite(tv)]
    return {"not_finite": int(tv.size - fin.size), "mean": float(fin.mean()),
            "quantiles": dict(zip((f"{v:g}" for v in QUANTILES), np.quantile(fin, QUANTILES).tolist()))}


def ktime_of(fam, fn):
    rtmi.ktime_enable(True)
    out = fn()
    ms = rtmi.ktime_read()[fam][0]
    rtmi.ktime_enable(False)
    return ms, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=sorted(rtmi.CAMERAS))
    ap.add_argument("--spp", type=int, default=64, help="bake: paths per sector")
    ap.add_argument("--split", type=int, default=4, help="bake: spp_split")
    ap.add_argument("--render-spp", type=int, default=128)
    ap.add_argument("--train", type=int, default=8, help="frames the trained map learns before it is frozen")
    ap.add_argument("--size", type=int, default=256, help="image size of the compared renders")
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--frame-time", action="store_true")
    ap.add_argument("--frame-size", type=int, default=512)
    ap.add_argument("--frame-spp", type=int, default=256)
    args = ap.parse_args()
    S = rtmi.sarsa
    g = load_scene(args.scene)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    gp = lambda **kw: rtmi.default_params(rtmi.RT_PRESET_GPU, seed=args.seed, **kw)  # noqa: E731
    p = gp(width=args.size, height=args.size, spp=args.render_spp, spp_split=8 if args.render_spp % 8 == 0 else 1)
    pb = gp(spp=args.spp, spp_split=args.split, t_scale=float(args.size))
    out = {"scene": args.scene, "size": args.size, "render_spp": args.render_spp, "ref_spp": args.ref_spp,
           "bake_spp": args.spp, "bake_split": args.split, "train_frames": args.train}
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc:
        ref, _ = rtmi.render(ctx, sc, cam, gp(width=args.size, height=args.size, spp=args.ref_spp, spp_split=8))
        out["default"] = errors(ref, rtmi.render(ctx, sc, cam, p)[0])
        with S.RadianceMap(ctx, sc, args.seed) as rm:
            if args.train > 0:
                rm.render(cam, p, args.train)
            rm.set_td_mode(S.TD_OFF)
            out["trained"] = errors(ref, rm.render(cam, p)[0])
            tv_trained = map_tv(ctx, sc, rm, pb, args.spp)
        with S.RadianceMap(ctx, sc, args.seed) as rm:
            secs, kms, casts = [], [], 0
            for _ in range(args.runs):
                t0 = time.perf_counter()
                ms, casts = ktime_of(rtmi.RT_KT_BAKE, lambda: rm.bake(sc, pb))
                secs.append(time.perf_counter() - t0)
                kms.append(ms)
            paths = rm.n_volumes * S.SECTORS * args.spp
            out["bake"] = {"volumes": rm.n_volumes, "paths": paths, "casts": casts, "seconds": secs, "k_bake_ms": kms,
                           "paths_per_s": paths / min(secs), "casts_per_s": casts / min(secs)}
            rm.set_td_mode(S.TD_OFF)
            out["baked"] = errors(ref, rm.render(cam, p)[0])
            p1 = gp(width=args.size, height=args.size, spp=1)
            out["irradiance"] = {name: errors(ref, rm.irradiance_view(cam, p1, k, None, weight))
                                 for name, k, weight in (("k1_mean", 1, rtmi.RT_IRR_MEAN), ("k3_mean", 3, rtmi.RT_IRR_MEAN),
                                                         ("k8_cone", 8, rtmi.RT_IRR_CONE))}
            out["map_tv"] = {"baked": map_tv(ctx, sc, rm, pb, args.spp), "trained": tv_trained}
            if args.frame_time:
                pf = gp(width=args.frame_size, height=args.frame_size, spp=args.frame_spp, spp_split=8)
                q, _, vis, _ = rm.read()
                rm.render(cam, pf)  # warm-up
                ft = {"off": [], "frame": []}
                for _ in range(args.runs):
                    for name, mode in (("off", S.TD_OFF), ("frame", S.TD_FRAME)):
                        rm.write(q, vis)  # every timed frame samples the same baked map
                        rm.set_td_mode(mode)
                        ft[name].append(ktime_of(rtmi.RT_KT_SARSA_RENDER, lambda: rm.render(cam, pf))[0])
                out["frame_ms"] = {"size": args.frame_size, "spp": args.frame_spp, **ft}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
