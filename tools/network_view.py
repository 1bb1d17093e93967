#!/usr/bin/env python3
"""What a Q-network believes arrives at every camera hit, beside what a radiance map believes:
the thesis's neural_q_visualisation.png beside expected_sarsa_visualisation.png.

    python tools/network_view.py door_room --model assets/models/door_room_12_12.model [--train N]
                                 [--spp 4] [--width 720] [--tint] [--exposure X] [--out DIR]

Writes
    <scene>_network_view.png      the Q-network view (rt_render_dqn_view): the network's irradiance
                                  estimate sum_k Q_k c_k * luminance / pi * (2 pi / 144) per hit
    <scene>_map_view.png          the map's rt_render_irradiance (k = 1, mean) of the default map, or
                                  with --train N of a map trained N Expected-SARSA frames
    <scene>_network_map_diff.png  the absolute difference of the two
and prints rtmi.metrics' MAPE between the two views (the map's as the reference).  The two
are on one scale (include/rtmi.h): the difference shows where the network departs from the map.
Exposure: by default each view's own 99th percentile goes to white and the difference takes the
smaller of the two factors, all printed (a network trained on the reference's rewards, 200 x the
lights' luminance, is orders of magnitude above an untrained map); --exposure X puts the one
factor X on all three PNGs.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=sorted(s for s in rtmi.CAMERAS if s != "cornell"))
    ap.add_argument("--model", required=True, help="DyNet text model of the scene's network (tools/fit_q.py, neuralq_train.py)")
    ap.add_argument("--train", type=int, default=0, help="Expected-SARSA frames the map is trained before its view")
    ap.add_argument("--train-spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--spp", type=int, default=4, help="samples per pixel of the views")
    ap.add_argument("--tint", action="store_true", help="times the surfaces' colour instead of grey")
    ap.add_argument("--exposure", type=float, default=None, help="one factor on all three PNGs (default: per view)")
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    w, h = args.width, args.height or args.width
    g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", args.scene + ".obj"), args.scene)
    W, b = rtmi.dqn.split_layers(rtmi.dqn.read_dynet(args.model))
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    os.makedirs(args.out, exist_ok=True)
    p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=w, height=h, spp=args.spp, spp_split=1, seed=args.seed)
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc, rtmi.dqn.Dqn(ctx, g.nn_vertices, W, b) as net, \
            rtmi.sarsa.RadianceMap(ctx, sc, args.seed) as rm:
        if args.train > 0:
            pt = rtmi.default_params(rtmi.RT_PRESET_GPU, width=w, height=h, spp=args.train_spp, seed=args.seed)
            rm.render(cam, pt, args.train)
            print(f"map: {rm.n_volumes} volumes, trained {args.train} frames of {args.train_spp} spp")
        else:
            print(f"map: {rm.n_volumes} volumes, untrained")
        net_img = rtmi.dqn.render_view(ctx, sc, net, cam, p, tint=args.tint)
        map_img = rm.irradiance_view(cam, p, 1, None, rtmi.RT_IRR_MEAN, args.tint)
    diff = np.abs(net_img - map_img)

    def auto(img):
        top = float(np.percentile(img, 99))
        return 1.0 / top if top > 0 else 1.0

    e_net = auto(net_img) if args.exposure is None else args.exposure
    e_map = auto(map_img) if args.exposure is None else args.exposure
    print(f"network view: mean {net_img.mean():.4g}, exposure {e_net:.4g}; "
          f"map view: mean {map_img.mean():.4g}, exposure {e_map:.4g}")
    for name, img, e in (("network_view", net_img, e_net), ("map_view", map_img, e_map),
                         ("network_map_diff", diff, min(e_net, e_map))):
        path = os.path.join(args.out, f"{args.scene}_{name}.png")
        rtmi.save_png(path, rtmi.pack_argb(np.ascontiguousarray(img * np.float32(e), np.float32)))
        print("wrote", path)
    print(f"MAPE of the network's view against the map's: {rtmi.metrics.mape_f(map_img, net_img):.4f}")


if __name__ == "__main__":
    main()
