#!/usr/bin/env python3
"""Saved sector distributions drawn inside the scene: the thesis's expected_sarsa_visualisation.png,
neural_q_visualisation.png and true_distribution.png (the reference's RENDER_SAVED_RADIANCE_VOLUMES).

    python tools/glyph_view.py door_room --selected selected_sarsa.txt [selected_deep.txt selected_true.txt]
                               [--base render|albedo] [--diameter 0.15] [--shade] [--spp 16]
                               [--colours ratio|magnitude] [--width 720] [--out DIR]

Every file (rt_sarsa_save_selected, rt_dqn_save_selected, tools/true_distribution.py) gives one PNG,
<scene>_glyphs_<file stem>.png: each of its points as a hemisphere of 12 x 12 sectors (rt_glyphs_create,
rt_render_glyph_view), red where the distribution is largest and green where it is small (ratio), or the
CPU engine's grey (magnitude), drawn over the scene's default render at the same camera and spp
(--base render) or over its albedo (--base albedo).  The PNGs are also placed side by side in
<scene>_glyphs_panels.png: the three files give the thesis's three-panel comparison.
Per glyph the tool prints the pixels it covers and where its largest sector points.
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
    ap.add_argument("scene", choices=sorted(rtmi.CAMERAS))
    ap.add_argument("--selected", nargs="+", required=True, help="per-volume files: x y z nx ny nz d0 .. d143 per line")
    ap.add_argument("--base", choices=("render", "albedo"), default="render")
    ap.add_argument("--diameter", type=float, default=rtmi.glyphs.DIAMETER)
    ap.add_argument("--shade", action="store_true", help="darken the sectors that face away from the camera ray")
    ap.add_argument("--colours", choices=("ratio", "magnitude"), default="ratio")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    w, h = args.width, args.height or args.width
    if args.scene == "cornell":
        g = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
    else:
        g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", args.scene + ".obj"), args.scene)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene])
    p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=w, height=h, spp=args.spp, spp_split=1, seed=args.seed)
    p1 = rtmi.default_params(rtmi.RT_PRESET_GPU, width=w, height=h, spp=1, seed=args.seed)
    mode = rtmi.glyphs.RATIO if args.colours == "ratio" else rtmi.glyphs.MAGNITUDE
    os.makedirs(args.out, exist_ok=True)
    panels = []
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc:
        base = rtmi.render(ctx, sc, cam, p)[0] if args.base == "render" else None
        for path in args.selected:
            pos, nrm, val = rtmi.read_selected(path)
            _, qn = rtmi.glyph_mesh(pos, nrm, args.diameter)
            with rtmi.Glyphs(ctx, pos, nrm, val, args.diameter, mode) as gl:
                img = gl.view(sc, cam, p, base=base, shade=args.shade)
                glyph = gl.view(sc, cam, p1, aov=True)[2]
            stem = os.path.splitext(os.path.basename(path))[0]
            out = os.path.join(args.out, f"{args.scene}_glyphs_{stem}.png")
            rtmi.save_png(out, rtmi.pack_argb(img))
            panels.append(img)
            print(f"wrote {out}: {len(pos)} glyphs of radius {args.diameter:g} over the {args.base} base")
            for i in range(len(pos)):
                k = int(np.argmax(val[i]))
                print(f"  glyph {i} at ({pos[i][0]:.3f}, {pos[i][1]:.3f}, {pos[i][2]:.3f}): "
                      f"{int(np.count_nonzero(glyph == i))} pixels; largest sector ({k // 12}, {k % 12}), "
                      f"{val[i][k] / max(float(val[i].sum()), 1e-30):.3f} of the distribution, pointing "
                      f"({qn[i][k][0]:+.2f}, {qn[i][k][1]:+.2f}, {qn[i][k][2]:+.2f})")
    out = os.path.join(args.out, f"{args.scene}_glyphs_panels.png")
    rtmi.save_png(out, rtmi.pack_argb(np.ascontiguousarray(np.concatenate(panels, axis=1))))
    print(f"wrote {out}: {len(panels)} panel(s)")


if __name__ == "__main__":
    main()
