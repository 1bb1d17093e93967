#!/usr/bin/env python3
"""The glyph view kernel by its two glyph-cast routes, beside the radiance-map view of the same frame.

    python tools/bench_glyph_view.py [--width 720] [--spp 16] [--runs 9] [--counts 1,3,7,16,64]

Frames: door_room with the three glyphs of tests/golden/selected_sarsa_ref.txt at D = 0.15, and
Cornell with the seven-glyph set of tests/test_glyph_view.py.  Per frame, k_glyph_view's
milliseconds by rt_ktime (family RT_KT_SARSA_VIEW, each run in its own enable window) with the
glyph cast on the BVH and, RTMI_GLYPH_BVH=0, on the plain scan -- the two alternate run by run
after a warm-up of each, the median of --runs is reported with its range -- and k_sarsa_view's on
the same camera, size and spp as the yardstick.  Then the two routes over glyph sets of growing
size in Cornell (--counts; random points of the box, axis normals, D = 0.15): the crossover.
Every timed pair is first checked to give the same bytes.  Prints one JSON line.
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

CORNELL_SET = (((0.0, 1.0, -0.5), (0.0, -1.0, 0.0), 0.4), ((-0.6, 1.0, -0.8), (0.0, -1.0, 0.0), 0.4),
               ((0.5, 0.2, 1.0), (0.0, 0.0, -1.0), 0.4), ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.4),
               ((0.6, 1.0, 0.6), (0.0, -1.0, 0.0), 0.4), ((0.0, 0.0, -2.0), (0.0, 0.0, -1.0), 0.15),
               ((0.3, -1.0, 0.0), (0.0, 1.0, 0.0), 0.4))


def ktime_of(fn):
    rtmi.ktime_enable(True)
    fn()
    ms, n = rtmi.ktime_read()[rtmi.RT_KT_SARSA_VIEW]
    rtmi.ktime_enable(False)
    assert n == 1, n
    return ms


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def routes(gl, sc, cam, p, runs):
    """k_glyph_view on the BVH and on the scan, alternating; the images must agree."""
    def view(route):
        if route == "scan":
            os.environ["RTMI_GLYPH_BVH"] = "0"
        try:
            return gl.view(sc, cam, p)
        finally:
            os.environ.pop("RTMI_GLYPH_BVH", None)

    a, b = view("bvh"), view("scan")  # warm-ups
    assert a.tobytes() == b.tobytes(), "the routes differ"
    ms = {"bvh": [], "scan": []}
    for _ in range(runs):
        for route in ("bvh", "scan"):
            ms[route].append(ktime_of(lambda: view(route)))
    return {k: summary(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--counts", default="1,3,7,16,64")
    args = ap.parse_args()
    W = H = args.width
    rng = np.random.default_rng(1984)
    result = {"width": W, "height": H, "spp": args.spp, "runs": args.runs, "frames": {}, "crossover": {}}
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)
    with rtmi.Context(0) as ctx:
        for scene in ("door_room", "cornell"):
            if scene == "cornell":
                g = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
                pos = np.array([s[0] for s in CORNELL_SET], np.float32)
                nrm = np.array([s[1] for s in CORNELL_SET], np.float32)
                diam = np.array([s[2] for s in CORNELL_SET], np.float32)
                val = rng.random((len(pos), 144), dtype=np.float32)
            else:
                g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", scene + ".obj"), scene)
                pos, nrm, val = rtmi.read_selected(os.path.join(ROOT, "tests", "golden", "selected_sarsa_ref.txt"))
                diam = 0.15
            cam = rtmi.camera(rtmi.CAMERAS[scene])
            p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=W, height=H, spp=args.spp, spp_split=1)
            with rtmi.Scene(ctx, g) as sc, rtmi.Glyphs(ctx, pos, nrm, val, diam) as gl, \
                    rtmi.sarsa.RadianceMap(ctx, sc, 1984) as rm:
                frame = routes(gl, sc, cam, p, args.runs)
                rm.view(cam, p)  # warm-up
                frame["k_sarsa_view"] = summary([ktime_of(lambda: rm.view(cam, p)) for _ in range(args.runs)])
                frame["glyphs"] = gl.info()
                glyph = gl.view(sc, cam, rtmi.default_params(rtmi.RT_PRESET_GPU, width=W, height=H, spp=1), aov=True)[2]
                frame["glyph_pixels"] = int(np.count_nonzero(glyph >= 0))
                result["frames"][scene] = frame
                if scene != "cornell":
                    continue
                for n in [int(c) for c in args.counts.split(",") if c]:
                    cp = rng.uniform(-0.9, 0.9, (n, 3)).astype(np.float32)
                    cn = axes[rng.integers(0, 6, n)]
                    with rtmi.Glyphs(ctx, cp, cn, rng.random((n, 144), dtype=np.float32), 0.15) as gc:
                        r = routes(gc, sc, cam, p, max(3, args.runs // 3))
                        r["glyphs"] = gc.info()
                        result["crossover"][str(n)] = r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
