#!/usr/bin/env python3
"""The thesis's fig:1_spp_max_dir (4_critical_evaluation.tex): a 1-spp frame in which every bounce
leaves in the direction of highest estimated radiance, for the radiance map and for the
Q-network, beside the reference image.

    python tools/max_direction.py door_room --model assets/models/door_room_12_12.model [--train N]
                                  [--ref-spp 256] [--width 720] [--exposure X] [--out DIR]

Three renders of one camera:
    <scene>_reference.png        the default (uniform) render at --ref-spp samples
    <scene>_map_max_dir.png      the radiance map after --train Expected-SARSA frames, 1 spp in
                                 RT_SARSA_SAMPLE_MAX (sample_max_direction_from_radiance_distribution)
    <scene>_network_max_dir.png  the network, 1 spp in RT_DQN_SAMPLE_MAX (sample_max_direction,
                                 nn_rendering_helpers.cu:491-553)
    <scene>_max_dir.png          the three side by side
and, as the thesis reads the figure, one line per method with the share of paths that contribute
nothing (throughput below 1e-4: they never reached a light) and the mean path length in ray
casts.  The max-direction estimators are biased on purpose (include/rtmi.h): the frames show
where each learner points, not a converged image.
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
    ap.add_argument("--model", required=True, help="DyNet text model of the scene's network")
    ap.add_argument("--train", type=int, default=10, help="Expected-SARSA frames the map is trained first")
    ap.add_argument("--train-spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--exposure", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    w, h = args.width, args.height or args.width
    g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", args.scene + ".obj"), args.scene)
    W, b = rtmi.dqn.split_layers(rtmi.dqn.read_dynet(args.model))
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    os.makedirs(args.out, exist_ok=True)
    p1 = rtmi.default_params(rtmi.RT_PRESET_GPU, width=w, height=h, spp=1, spp_split=1, seed=args.seed)
    pr = rtmi.default_params(rtmi.RT_PRESET_GPU, width=w, height=h, spp=args.ref_spp, seed=args.seed)
    pt = rtmi.default_params(rtmi.RT_PRESET_GPU, width=w, height=h, spp=args.train_spp, seed=args.seed)
    pixels = w * h
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc, rtmi.dqn.Dqn(ctx, g.nn_vertices, W, b) as net, \
            rtmi.sarsa.RadianceMap(ctx, sc, args.seed) as rm:
        ref, ref_casts = rtmi.render(ctx, sc, cam, pr)
        if args.train > 0:
            rm.render(cam, pt, args.train)
        rm.set_sampling(rtmi.sarsa.SAMPLE_MAX)
        map_img, map_casts = rm.render(cam, p1, 1)
        _, map_zero = rm.frame_stats()
        net.set_sampling(net.SAMPLE_MAX)
        rtmi.dqn.enable_stats(ctx, True)
        net_img, net_casts = rtmi.dqn.render(ctx, sc, net, cam, p1)
        net_paths, net_zero = rtmi.dqn.render_stats(ctx)
    print(f"reference: {args.ref_spp} spp, mean path length {ref_casts / (pixels * args.ref_spp):.2f}")
    print(f"map (trained {args.train} frames): zero-contribution paths {map_zero / pixels:.4f}, "
          f"mean path length {map_casts / pixels:.2f}")
    print(f"network ({os.path.basename(args.model)}): zero-contribution paths {net_zero / net_paths:.4f}, "
          f"mean path length {net_casts / net_paths:.2f}")
    e = np.float32(args.exposure)
    panels = []
    for name, img in (("reference", ref), ("map_max_dir", map_img), ("network_max_dir", net_img)):
        img = np.nan_to_num(np.ascontiguousarray(img * e, np.float32), nan=0.0, posinf=1.0, neginf=0.0)
        panels.append(img)
        path = os.path.join(args.out, f"{args.scene}_{name}.png")
        rtmi.save_png(path, rtmi.pack_argb(img))
        print("wrote", path)
    path = os.path.join(args.out, f"{args.scene}_max_dir.png")
    rtmi.save_png(path, rtmi.pack_argb(np.ascontiguousarray(np.concatenate(panels, axis=1))))
    print("wrote", path)


if __name__ == "__main__":
    main()
