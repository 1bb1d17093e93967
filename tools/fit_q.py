#!/usr/bin/env python3
"""Fit the Q-network to a radiance map: the reference's NN_Q_Value_Trainer on the device.

    python tools/fit_q.py door_room --train 4 --epochs 100 --out door_room_fit.model
                          [--q-table FILE] [--render] [--batch 128] [--size 256] [--spp 16]

1. The data: an Expected-SARSA radiance map of the scene learned for --train frames
   (rt_render_sarsa at --size, --spp), or a saved radiance_map_data.txt (--q-table, the file
   of RadianceMap.save_q / the reference's save_q_vals_to_file).
2. The network: 200-300-200 ReLU from rtmi.dqn.glorot_weights (DyNet's default initialiser).
3. The fit: rtmi.dqn.QFit, --epochs epochs of batches of --batch rows over an 80/20 split; the
   reference's per-epoch block (NN_Q_Value_Trainer/Source/main.cu:279-283) goes to stdout.
4. The DyNet .model out (rtmi.dqn.write_dynet), which rt_render_dqn / the reference's
   PretrainedPathtracer load.
5. --render: the fitted network's render (rtmi.dqn.render) beside the map's own render of the
   same frame, and the MAPE between the two (rtmi.metrics.mape_f).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", help="door_room, archway, complex_light_room or cornell")
    ap.add_argument("--train", type=int, default=4, help="radiance-map frames before the fit")
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--out", default=None, help="DyNet .model (default <scene>_fit.model)")
    ap.add_argument("--q-table", default=None, help="a saved radiance_map_data.txt instead of a learned map")
    ap.add_argument("--render", action="store_true")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    args = ap.parse_args()
    out = args.out or args.scene + "_fit.model"
    if args.scene == "cornell":
        g = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
    else:
        g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", args.scene + ".obj"), args.scene)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=args.size, height=args.size, spp=args.spp)
    W, b = rtmi.dqn.glorot_weights(g.nn_vertices.size, seed=args.seed)
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc:
        rm = None
        if args.q_table is None or args.render:
            rm = rtmi.sarsa.RadianceMap(ctx, sc, args.seed)
            if args.q_table is not None:
                rm.load_q(args.q_table)
            elif args.train > 0:
                rm.render(cam, p, args.train)
        with rtmi.dqn.DqnTrainer(ctx, g.nn_vertices, W, b, learning_rate=args.lr) as tr:
            kw = dict(seed=args.seed, batch_size=args.batch)
            if args.q_table is not None:
                fit = rtmi.dqn.QFit.from_file(ctx, tr, args.q_table, **kw)
            else:
                fit = rtmi.dqn.QFit.from_map(ctx, tr, rm, **kw)
            with fit:
                info = fit.info()
                print(f"Training data set size: {info['n_train']}\nTest data set size: {info['n_test']}", flush=True)
                for i in range(args.epochs):
                    loss, error = fit.epoch()
                    sys.stdout.write(rtmi.dqn.QFit.epoch_block(i + 1, loss, error))
                    sys.stdout.flush()
            Wf, bf = tr.params()
        rtmi.dqn.write_dynet(out, rtmi.dqn.join_layers(Wf, bf))
        print(f"wrote {out}")
        if args.render:
            with rtmi.dqn.Dqn(ctx, g.nn_vertices, Wf, bf) as net:
                img_net, casts_net = rtmi.dqn.render(ctx, sc, net, cam, p)
            img_map, casts_map = rm.render(cam, p, 1)
            stem = os.path.splitext(out)[0]
            for name, img in (("fit", img_net), ("map", img_map)):
                rtmi.save_png(f"{stem}_{name}.png", rtmi.pack_argb(img))
            print(f"render: network {casts_net} ray casts -> {stem}_fit.png, map {casts_map} ray casts -> "
                  f"{stem}_map.png, MAPE(map, network) {rtmi.metrics.mape_f(img_map, img_net):.4f}")
        if rm is not None:
            rm.close()


if __name__ == "__main__":
    main()
