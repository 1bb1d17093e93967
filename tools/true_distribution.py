#!/usr/bin/env python3
"""The true incident radiance distribution at selected points, beside what was learned there:
the first column of the thesis's figure (4_critical_evaluation.tex:92-110, true_distribution.png;
"4096 sampled light paths per sector"), whose other two are selected_sarsa.txt and
selected_deep.txt.

    python tools/true_distribution.py door_room [--train N] [--model FILE] [--spp 4096]
    python tools/true_distribution.py door_room --train N --all-volumes --spp 64

Builds the scene's radiance map and optionally trains it N Expected-SARSA frames.  For each row
"x y z nx ny nz" of --to-select it takes the nearest volume's position and surface, as
rt_sarsa_save_selected does, probes that volume (rt_probe_radiance, the volume's index as its RNG
identity) and writes --out in the format of selected_sarsa.txt: "x y z nx ny nz d0 .. d143", d the
normalised luminance per sector.  It prints the error of the map's normalised Q against the truth
per point (total variation, KL divergence: rtmi.probe.distribution_error), and the network's
normalised Q with --model (a DyNet text model of the scene).  --all-volumes probes every volume
of the map instead, in batches, and prints the quantiles of the map's error over the map.
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

QUANTILES = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)


def load_scene(name):
    if name == "cornell":
        return rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
    return rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", name + ".obj"), name)


def read_locations(path):
    rows = [np.array(l.split(), np.float64) for l in open(path) if l.strip()]
    a = np.array(rows, np.float32).reshape(len(rows), 6)
    return a[:, :3].copy(), a[:, 3:].copy()


def quantiles(x):
    x = np.asarray(x, np.float64)
    fin = x[np.isfinite(x)]
    q = np.quantile(fin, QUANTILES).tolist() if fin.size else [float("nan")] * len(QUANTILES)
    return {"n": int(x.size), "not_finite": int(x.size - fin.size), "mean": float(fin.mean()) if fin.size else None,
            "quantiles": dict(zip((f"{v:g}" for v in QUANTILES), q))}


def pick_split(n_points, spp, items=1 << 21):
    split = 1
    while spp % (2 * split) == 0 and n_points * rtmi.probe.SECTORS * split < items:
        split *= 2
    return split


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=sorted(rtmi.CAMERAS))
    ap.add_argument("--train", type=int, default=0, help="Expected-SARSA frames rendered before the probe")
    ap.add_argument("--train-spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=512, help="image size of the training frames")
    ap.add_argument("--model", default=None, help="a DyNet text model of the scene's Q-network")
    ap.add_argument("--spp", type=int, default=4096, help="paths per sector")
    ap.add_argument("--split", type=int, default=0,
                    help="spp_split, part of the result's definition (default: the smallest power of two dividing "
                         "spp that gives a call 2^21 (point, sector, chunk) items, enough lanes to fill the device)")
    ap.add_argument("--max-bounces", type=int, default=None, help="default: the GPU preset's 80")
    ap.add_argument("--all-volumes", action="store_true", help="every volume of the map, error quantiles")
    ap.add_argument("--batch", type=int, default=4096, help="volumes per call with --all-volumes")
    ap.add_argument("--to-select", default=os.path.join(ROOT, "tests", "golden", "to_select.txt"))
    ap.add_argument("--out", default="selected_true.txt")
    ap.add_argument("--seed", type=int, default=1984)
    args = ap.parse_args()
    g = load_scene(args.scene)
    P, S = rtmi.probe, rtmi.sarsa
    kw = {} if args.max_bounces is None else {"max_bounces": args.max_bounces}
    p = rtmi.default_params(rtmi.RT_PRESET_GPU, spp=args.spp, spp_split=args.split or 1, seed=args.seed, **kw)
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc, S.RadianceMap(ctx, sc, args.seed) as rm:
        print(f"{args.scene}: {rm.n_volumes} radiance volumes")
        if args.train > 0:
            pt = rtmi.default_params(rtmi.RT_PRESET_GPU, width=args.width, height=args.width, spp=args.train_spp,
                                     seed=args.seed)
            rm.render(rtmi.camera(rtmi.CAMERAS[args.scene]), pt, args.train)
            print(f"trained {args.train} frames of {args.train_spp} spp at {args.width}^2")
        vpos, vnrm, vsurf, _ = rm.volumes()
        q_map = rm.read()[0]
        if args.all_volumes:
            split = p.spp_split = args.split or pick_split(min(args.batch, rm.n_volumes), args.spp)
            tv, kl = [], []
            casts, t0 = 0, time.perf_counter()
            for b in range(0, rm.n_volumes, args.batch):
                idx = np.arange(b, min(b + args.batch, rm.n_volumes))
                got = P.radiance(ctx, sc, p, vpos[idx], vsurf[idx], idx, want_irr=False)
                e = P.distribution_error(P.distribution(got["rad"]), q_map[idx])
                tv.append(e["tv"])
                kl.append(e["kl"])
                casts += got["casts"]
            dt = time.perf_counter() - t0
            paths = rm.n_volumes * P.SECTORS * args.spp
            print(json.dumps({"scene": args.scene, "volumes": rm.n_volumes, "trained_frames": args.train,
                              "spp": args.spp, "spp_split": split, "max_bounces": p.max_bounces, "paths": paths,
                              "casts": casts, "seconds": dt, "paths_per_s": paths / dt,
                              "map_tv": quantiles(np.concatenate(tv)), "map_kl": quantiles(np.concatenate(kl))}))
            return
        loc, nrm = read_locations(args.to_select)
        idx = rm.nearest(loc, nrm)
        p.spp_split = args.split or pick_split(len(idx), args.spp)
        t0 = time.perf_counter()
        got = P.radiance(ctx, sc, p, vpos[idx], vsurf[idx], idx, want_irr=False)
        dt = time.perf_counter() - t0
        true = P.distribution(got["rad"])
        P.write_selected_file(args.out, vpos[idx], vnrm[idx], true)
        paths = len(idx) * P.SECTORS * args.spp
        print(f"wrote {args.out}: {len(idx)} points x {P.SECTORS} sectors x {args.spp} paths (spp_split {p.spp_split}), "
              f"{got['casts']} casts, {dt:.3f} s ({paths / dt:.3e} paths/s)")
        cols = {"map": P.distribution_error(true, q_map[idx])}
        if args.model:
            W, b = rtmi.dqn.split_layers(rtmi.dqn.read_dynet(args.model))
            with rtmi.dqn.Dqn(ctx, g.nn_vertices, W, b) as net:
                cols["network"] = P.distribution_error(true, np.maximum(net.forward(vpos[idx]), 0.0))
        for i, v in enumerate(idx):
            line = f"point {i}: volume {int(v)} at ({vpos[v][0]:g} {vpos[v][1]:g} {vpos[v][2]:g})"
            for name, e in cols.items():
                line += f"  {name}: tv {e['tv'][i]:.4f} kl {e['kl'][i]:.4f}"
            print(line)


if __name__ == "__main__":
    main()
