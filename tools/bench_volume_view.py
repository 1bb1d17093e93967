#!/usr/bin/env python3
"""The radiance-map view kernel against the same work through the older entry points.

    python tools/bench_volume_view.py [--scene door_room] [--width 720] [--runs 11]

Per spp in (1, 16): k_sarsa_view timed by rt_ktime (a warm-up run, then the median of --runs
runs), and beside it, in the same process and on the same map, the pair it fuses:
rt_intersect_device on the view's camera rays (HIP events on its stream), then
rt_sarsa_nearest on the surface hit points (k_sarsa_nearest by rt_ktime, without the call's
copies, and the whole call by the wall clock).  The rays are rebuilt from the view's own hit
points (direction = normalised hit point - camera; a pixel without a surface hit takes its
centre's direction), so they are the view's rays up to rounding.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd"))
import rtmi  # noqa: E402


def ktime_of(fam, fn):
    rtmi.ktime_enable(True)
    fn()
    ms, n = rtmi.ktime_read()[fam]
    rtmi.ktime_enable(False)
    return ms, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="door_room")
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--search", choices=("grid", "kd"), default="grid")
    ap.add_argument("--split", type=int, default=1, help="spp_split of the spp-16 view")
    ap.add_argument("--yaw-x", type=float, default=0.0, help="camera pitch (non-zero: the scan, no rectangle cull)")
    ap.add_argument("--view-only", action="store_true", help="skip the intersect + nearest pair")
    args = ap.parse_args()
    W = H = args.width
    if args.scene == "cornell":
        g = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
    else:
        g = rtmi.obj_geometry(os.path.join(ROOT, "assets", "models", args.scene + ".obj"), args.scene)
    cam = rtmi.camera(rtmi.CAMERAS[args.scene], yaw_x=args.yaw_x)
    o = np.array(rtmi.CAMERAS[args.scene][:3], np.float32)
    S = rtmi.sarsa
    dev = torch.device("cuda", 0)
    result = {"scene": args.scene, "width": W, "height": H, "runs": args.runs, "search": args.search, "split16": args.split,
              "yaw_x": args.yaw_x, "spp": {}}
    with rtmi.Context(0) as ctx, rtmi.Scene(ctx, g) as sc, S.RadianceMap(ctx, sc, 1984) as rm:
        rm.set_search(S.SEARCH_GRID if args.search == "grid" else S.SEARCH_KD)
        result["volumes"] = rm.n_volumes
        p1 = rtmi.default_params(rtmi.RT_PRESET_GPU, width=W, height=H, spp=1)
        normals = sc.normals()
        px, py = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
        centre = np.stack([px + 0.5 - W / 2, py + 0.5 - H / 2, np.full_like(px, H)], 2).astype(np.float32)
        for spp in (1, 16):
            p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=W, height=H, spp=spp,
                                    spp_split=args.split if spp > 1 else 1)
            rm.view(cam, p)  # warm-up
            view_ms = [ktime_of(rtmi.RT_KT_SARSA_VIEW, lambda: rm.view(cam, p))[0] for _ in range(args.runs)]
            if args.view_only:
                result["spp"][str(spp)] = {"view_kernel_ms": statistics.median(view_ms)}
                continue
            # the same samples' rays and hit points, from spp single-sample views
            dirs, pts, nrm = [], [], []
            for s in range(spp):
                _, tri, vol, pos = rm.view(cam, p1, s, aov=True)
                surf = vol >= 0
                d = np.where(surf[:, :, None], pos - o, centre)
                d /= np.linalg.norm(d, axis=2, keepdims=True)
                dirs.append(d.reshape(-1, 3).astype(np.float32))
                pts.append(pos[surf])
                nrm.append(normals[tri[surf]])
            d_all, pts, nrm = np.concatenate(dirs), np.concatenate(pts), np.concatenate(nrm)
            n = d_all.shape[0]
            t_o = torch.from_numpy(np.broadcast_to(o, d_all.shape).copy()).to(dev)
            t_d = torch.from_numpy(d_all).to(dev)
            t_t = torch.zeros(n, dtype=torch.float32, device=dev)
            t_h = torch.zeros(n, dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream()

            def isect():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rtmi.intersect_device(ctx, sc, t_o.data_ptr(), t_d.data_ptr(), n, p.t_scale, p.hit_rule,
                                      t_t.data_ptr(), t_h.data_ptr(), stream.cuda_stream)
                e1.record(stream)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            isect()
            rm.nearest(pts, nrm)  # warm-ups
            isect_ms = [isect() for _ in range(args.runs)]
            near_ms, near_wall = [], []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                ms, _ = ktime_of(rtmi.RT_KT_SARSA_NEAREST, lambda: rm.nearest(pts, nrm))
                near_wall.append((time.perf_counter() - t0) * 1e3)
                near_ms.append(ms)
            med = statistics.median
            result["spp"][str(spp)] = {
                "rays": n, "surface_hits": int(pts.shape[0]),
                "view_kernel_ms": med(view_ms), "view_kernel_ms_min_max": [min(view_ms), max(view_ms)],
                "intersect_device_ms": med(isect_ms), "nearest_kernel_ms": med(near_ms),
                "pair_kernels_ms": med(isect_ms) + med(near_ms), "nearest_call_wall_ms": med(near_wall),
            }
        result["kd_fallbacks"] = rm.search_stats()["kd_fallbacks"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
