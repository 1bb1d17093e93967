"""Expected-SARSA radiance volumes (BASELINE config 3) on top of the C ABI.

  RadianceMap(ctx, scene, seed)   rt_sarsa_create: volumes, Q-table, KD tree on the device
  RadianceMap(..., area_per_sample=a)   rt_sarsa_create_density: another AREA_PER_SAMPLE
  .render(cam, params, frames)    draw_reinforcement_path_tracing + update_radiance_volume_
                                  distributions per frame (rt_render_sarsa)
  .render_tiles_device(...)       one frame over a tile list; apply=False leaves the frame's TD
                                  sums for a cross-GPU sum (rtmi.dist.sarsa_frame)
  .read() / .volumes() / .nearest(pos, nrm)   Q-table, placement, KD queries (parity)
  .save_q(path) / .load_q(path)   radiance_map_data.txt out and back in (resume a trained map)
  read_q(path)                    such a file without a map: (positions, Q) for rtmi.dqn.QFit
  .set_sampling(SAMPLE_MAX)      sample_max_direction_from_radiance_distribution
  .set_td_mode(TD_INFRAME)        the reference's racy in-frame TD update (one GPU)
  .set_td_mode(TD_OFF)            render from the map as it stands, learning nothing
  .bake(scene, params, v0, n)     fill volumes from ground truth on the device (rt_sarsa_bake)
  .write(q, visits, v0)           Q rows (and visits) from host arrays into the map (rt_sarsa_write)
  .sweep(scene, params, v0, n)    one expected-value sweep: the TD target of every sector from the volume's
                                  own position, value iteration over the map (rt_sarsa_sweep)
  .forget(v0, n)                  visits = 0: the next applied targets replace Q (rt_sarsa_forget)
  .frame_stats() / .append_stats_line(path)   sarsa_training_stats.txt (GPU/main.cu:321-339)
  .view(cam, params, first_sample, aov) / .view_tiles_device(...)   the Voronoi view (GPU/main.cu
                                  method 2): each camera hit in its nearest volume's colour
  .knn(pos, nrm, k, radius) / .knn_reach()   the k nearest same-normal volumes within radius (rt_sarsa_knn)
  .irradiance_view(cam, params, k, radius, weight, tint) / .irradiance_view_tiles_device(...)   the CPU
                                  engine's draw_radiance_map_path_tracing: each camera hit as the map's
                                  irradiance estimate there, interpolated over the k nearest volumes
  .set_view_colours(rgb)          the view's per-volume colours; voronoi_palette(seed, n) the default,
                                  irradiance_colours / visits_colours / max_q_colours from read()
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._lib import RT_IRR_CONE, RT_IRR_MEAN, RT_SARSA_KNN_MAX, RtIrrOpts, check, lib

from .api import Context, Scene, _fp, _ip

SEARCH_KD = 0    # RT_SARSA_SEARCH_KD
SEARCH_GRID = 1  # RT_SARSA_SEARCH_GRID
SAMPLE_CDF = 0   # RT_SARSA_SAMPLE_CDF
SAMPLE_MAX = 1   # RT_SARSA_SAMPLE_MAX
TD_FRAME = 0     # RT_SARSA_TD_FRAME
TD_INFRAME = 1   # RT_SARSA_TD_INFRAME
TD_OFF = 2       # RT_SARSA_TD_OFF

SECTORS = 144  # GRID_RESOLUTION^2

KD_DTYPE = np.dtype([("dim", "<i4"), ("leaf", "<i4"), ("left", "<i4"), ("right", "<i4"), ("data", "<f4"),
                     ("px", "<f4"), ("py", "<f4"), ("pz", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                     ("vol", "<i4")])


class RadianceMap:
    def __init__(self, ctx: Context, scene: Scene, seed: int = 1984, area_per_sample: float | None = None):
        """area_per_sample: the volume density, floor(area / area_per_sample) volumes per
        surface (AREA_PER_SAMPLE, radiance_volumes_settings.h:12; None = the reference's 0.001)"""
        self.ctx = ctx
        self.scene = scene
        self._h = ctypes.c_void_p()
        if area_per_sample is None:
            check(lib().rt_sarsa_create(ctx.handle, scene.handle, seed, ctypes.byref(self._h)))
        else:
            check(lib().rt_sarsa_create_density(ctx.handle, scene.handle, seed, float(area_per_sample),
                                                ctypes.byref(self._h)))
        nv, nk, fr = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_uint32(0)
        check(lib().rt_sarsa_info(self._h, ctypes.byref(nv), ctypes.byref(nk), ctypes.byref(fr)))
        self.n_volumes, self.n_nodes = nv.value, nk.value

    @property
    def handle(self):
        return self._h

    @property
    def frames(self) -> int:
        fr = ctypes.c_uint32(0)
        check(lib().rt_sarsa_info(self._h, None, None, ctypes.byref(fr)))
        return int(fr.value)

    def set_search(self, mode: int) -> None:
        """RT_SARSA_SEARCH_KD (0) or RT_SARSA_SEARCH_GRID (1, default); same results."""
        check(lib().rt_sarsa_set_search(self._h, mode))

    def search_stats(self) -> dict:
        mode, ncls = ctypes.c_int32(0), ctypes.c_int32(0)
        cells, fb = ctypes.c_int64(0), ctypes.c_uint64(0)
        check(lib().rt_sarsa_search_stats(self._h, ctypes.byref(mode), ctypes.byref(ncls), ctypes.byref(cells),
                                          ctypes.byref(fb)))
        return {"mode": int(mode.value), "classes": int(ncls.value), "grid_cells": int(cells.value),
                "kd_fallbacks": int(fb.value)}

    def save_q(self, path: str) -> None:
        """radiance_map_data.txt format (RadianceMap::save_q_vals_to_file)."""
        check(lib().rt_sarsa_save_q(self._h, os.fsencode(path)))

    def load_q(self, path: str) -> None:
        """A radiance_map_data.txt of this map (same scene and seed) back into the device map:
        Q from the file, irradiance estimate and CDF recomputed, visits kept (rt_sarsa_load_q)."""
        check(lib().rt_sarsa_load_q(self._h, os.fsencode(path)))

    def set_sampling(self, mode: int) -> None:
        """SAMPLE_CDF (default) or SAMPLE_MAX (the sector of largest Q, radiance_volume.cu:246-278)."""
        check(lib().rt_sarsa_set_sampling(self._h, mode))

    def set_td_mode(self, mode: int) -> None:
        """TD_FRAME (default: frame-synchronous, deterministic), TD_INFRAME (the reference's
        in-frame read-modify-write, radiance_volume.cu:282-301; racy, one GPU only) or TD_OFF
        (a frozen map: frames sample it and change nothing in it)."""
        check(lib().rt_sarsa_set_td_mode(self._h, mode))

    def set_inframe_lanes(self, lanes: int) -> None:
        """paths in flight of the in-frame rule's render (0: the device's full occupancy;
        the reference's GTX 1070 Ti holds 38,912): rt_sarsa_set_inframe_lanes"""
        check(lib().rt_sarsa_set_inframe_lanes(self._h, lanes))

    @property
    def td_mode(self) -> int:
        """the map's TD rule, read from the library (rt_sarsa_get_td_mode)"""
        m = ctypes.c_int32(0)
        check(lib().rt_sarsa_get_td_mode(self._h, ctypes.byref(m)))
        return int(m.value)

    def frame_stats(self):
        """(sum over pixels of int(mean path length), zero-contribution paths) of the last frame."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib().rt_sarsa_frame_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def append_stats_line(self, path: str, pixels: int, sums=None) -> str:
        """One line of sarsa_training_stats.txt (GPU/main.cu:330-339): the average path length
        (integer division over `pixels`, printed as the float it is stored in), 0.0, the
        zero-contribution paths.  sums: (path_floor_sum, zero_paths) summed over ranks, else
        this map's frame_stats()."""
        paths, zero = self.frame_stats() if sums is None else sums
        line = stats_line(paths, zero, pixels)
        with open(path, "a") as fh:
            fh.write(line)
        return line

    def save_selected(self, to_select: str, out: str) -> None:
        """selected_sarsa.txt format for the locations of to_select.txt."""
        check(lib().rt_sarsa_save_selected(self.ctx.handle, self._h, os.fsencode(to_select), os.fsencode(out)))

    def volumes(self):
        n = self.n_volumes
        pos = np.zeros((n, 3), np.float32)
        nrm = np.zeros((n, 3), np.float32)
        surf = np.zeros(n, np.int32)
        kd = np.zeros(self.n_nodes, KD_DTYPE)
        check(lib().rt_sarsa_volumes(self._h, _fp(pos), _fp(nrm), _ip(surf), kd.ctypes.data_as(ctypes.c_void_p)))
        return pos, nrm, surf, kd

    def read(self):
        """(Q, CDF, visits) as n x 144 and the irradiance estimate accumulators (n)."""
        n = self.n_volumes
        q = np.zeros((n, SECTORS), np.float32)
        cdf = np.zeros((n, SECTORS), np.float32)
        vis = np.zeros((n, SECTORS), np.uint32)
        acc = np.zeros(n, np.float32)
        check(lib().rt_sarsa_read(self._h, _fp(q), _fp(cdf), vis.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                  _fp(acc)))
        return q, cdf, vis, acc

    def write(self, q, visits=None, v0: int = 0) -> None:
        """The counterpart of read(): Q rows (n, 144) into the volumes [v0, v0 + n); the irradiance
        estimate and the CDF are recomputed as load_q does; visits (n, 144) are set, or kept when
        None (rt_sarsa_write)."""
        qa = np.ascontiguousarray(q, np.float32)
        if qa.ndim != 2 or qa.shape[1] != SECTORS:
            raise ValueError(f"q must be (n, {SECTORS}), got {qa.shape}")
        va = None
        if visits is not None:
            va = np.ascontiguousarray(visits, np.uint32)
            if va.shape != qa.shape:
                raise ValueError(f"visits must be {qa.shape}, got {va.shape}")
        check(lib().rt_sarsa_write(self._h, int(v0), qa.shape[0], _fp(qa),
                                   None if va is None else va.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))

    def bake(self, scene: Scene, params, v0: int = 0, n: int | None = None, first_sample: int = 0) -> int:
        """Fill the volumes [v0, v0 + n) (n None: to the end of the map) from ground truth on the
        device: per sector the luminance of rtmi.probe.radiance at the volume, times the
        surface's luminance / pi, floored at RADIANCE_THRESHOLD; visits = spp; irradiance and CDF
        follow (rt_sarsa_bake).  Returns the closest-hit calls."""
        if n is None:
            n = self.n_volumes - int(v0)
        casts = ctypes.c_uint64(0)
        check(lib().rt_sarsa_bake(self.ctx.handle, scene.handle, self._h, ctypes.byref(params), int(v0), int(n),
                                  int(first_sample), ctypes.byref(casts), None))
        return int(casts.value)

    def sweep(self, scene: Scene, params, v0: int = 0, n: int | None = None, first_sample: int = 0,
              apply: bool = True) -> int:
        """One expected-value sweep of the volumes [v0, v0 + n) (n None: to the end of the map): per
        sector params.spp single casts from the volume's own position, each depositing the
        Expected-SARSA target (the light, or the map's irradiance estimate where the cast lands)
        into the pending TD sums; apply folds them into Q as a frame's are (rt_sarsa_sweep).  The
        map must be in TD_FRAME.  Returns the casts, n * 144 * spp."""
        if n is None:
            n = self.n_volumes - int(v0)
        casts = ctypes.c_uint64(0)
        check(lib().rt_sarsa_sweep(self.ctx.handle, scene.handle, self._h, ctypes.byref(params), int(v0), int(n),
                                   int(first_sample), int(bool(apply)), ctypes.byref(casts), None))
        return int(casts.value)

    def forget(self, v0: int = 0, n: int | None = None) -> None:
        """visits = 0 for the volumes [v0, v0 + n), nothing else: the next applied targets replace Q
        instead of joining its running mean (rt_sarsa_forget).  forget + sweep is a Jacobi step."""
        if n is None:
            n = self.n_volumes - int(v0)
        check(lib().rt_sarsa_forget(self._h, int(v0), int(n), None))

    def nearest(self, pos: np.ndarray, nrm: np.ndarray) -> np.ndarray:
        p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        n_ = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        out = np.zeros(p.shape[0], np.int32)
        check(lib().rt_sarsa_nearest(self.ctx.handle, self._h, _fp(p), _fp(n_), p.shape[0], _ip(out)))
        return out

    def render(self, cam, params, frames: int = 1):
        out = np.zeros((params.height, params.width, 3), np.float32)
        casts = ctypes.c_uint64(0)
        check(lib().rt_render_sarsa(self.ctx.handle, self.scene.handle, self._h, ctypes.byref(cam),
                                    ctypes.byref(params), frames, _fp(out), ctypes.byref(casts)))
        return out, int(casts.value)

    def render_tiles_device(self, cam, params, tiles: np.ndarray, tile_size: int, out_ptr: int, casts_ptr: int,
                            apply: bool, stream: int) -> None:
        t = np.ascontiguousarray(tiles, np.int32).reshape(-1, 2)
        check(lib().rt_render_sarsa_tiles_device(self.ctx.handle, self.scene.handle, self._h, ctypes.byref(cam),
                                                 ctypes.byref(params), _ip(t), t.shape[0], tile_size,
                                                 ctypes.c_void_p(out_ptr), ctypes.c_void_p(casts_ptr),
                                                 int(bool(apply)), ctypes.c_void_p(stream)))

    def set_view_colours(self, rgb=None) -> None:
        """The views' per-volume colour table, n_volumes x 3 (rt_sarsa_set_view_colours); None:
        the random palette of the map's seed (RadianceMap::set_voronoi_colours), which is also
        what a map that never had this called draws with."""
        if rgb is None:
            check(lib().rt_sarsa_set_view_colours(self._h, None))
            return
        t = np.ascontiguousarray(rgb, np.float32)
        if t.shape != (self.n_volumes, 3):
            raise ValueError(f"colour table must be ({self.n_volumes}, 3), got {t.shape}")
        check(lib().rt_sarsa_set_view_colours(self._h, _fp(t)))

    def view(self, cam, params, first_sample: int = 0, aov: bool = False):
        """Every camera hit in the colour of its nearest volume (the reference's Voronoi view,
        GPU/path_tracing/voronoi_trace.cu; rt_render_volume_view): samples first_sample ..
        first_sample + spp - 1 of rt_render_sarsa's camera rays.  The map is left as it is.
        Returns rgb (H, W, 3); with aov, (rgb, tri, vol, pos) where tri (-1 miss, >= n_surf
        light), vol (-1 unless a surface was hit) and pos (H, W, 3) describe sample first_sample."""
        h, w = params.height, params.width
        out = np.zeros((h, w, 3), np.float32)
        if not aov:
            check(lib().rt_render_volume_view(self.ctx.handle, self.scene.handle, self._h, ctypes.byref(cam),
                                              ctypes.byref(params), first_sample, _fp(out), None, None, None))
            return out
        tri = np.zeros((h, w), np.int32)
        vol = np.zeros((h, w), np.int32)
        pos = np.zeros((h, w, 3), np.float32)
        check(lib().rt_render_volume_view(self.ctx.handle, self.scene.handle, self._h, ctypes.byref(cam),
                                          ctypes.byref(params), first_sample, _fp(out), _ip(tri), _ip(vol), _fp(pos)))
        return out, tri, vol, pos

    def view_tiles_device(self, cam, params, tiles: np.ndarray, tile_size: int, out_ptr: int, stream: int,
                          first_sample: int = 0) -> None:
        """The view over a tile list into device memory, stream-ordered; tiles and output
        layout as render_tiles_device (rt_render_volume_view_tiles_device)."""
        t = np.ascontiguousarray(tiles, np.int32).reshape(-1, 2)
        check(lib().rt_render_volume_view_tiles_device(self.ctx.handle, self.scene.handle, self._h, ctypes.byref(cam),
                                                       ctypes.byref(params), first_sample, _ip(t), t.shape[0],
                                                       tile_size, ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream)))

    def knn_reach(self) -> float:
        """The largest radius knn() answers: the grid's accept radius, sqrt(MAX_DIST) * 0.999; 0
        for a map without a grid (rt_sarsa_knn_reach)."""
        r = ctypes.c_float(0)
        check(lib().rt_sarsa_knn_reach(self._h, ctypes.byref(r)))
        return float(r.value)

    def _irr_opts(self, k, radius, weight, tint) -> RtIrrOpts:
        return RtIrrOpts(int(k), self.knn_reach() if radius is None else float(radius), int(weight), int(bool(tint)))

    def knn(self, pos: np.ndarray, nrm: np.ndarray, k: int, radius: float | None = None):
        """Per query the volumes with its normal closer than radius (None: the reach), the k
        nearest ascending by (distance, index): (vol (n, k) int32, dist (n, k), count (n)); unused
        slots hold -1 and +inf (rt_sarsa_knn)."""
        p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        n_ = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        n, kk = p.shape[0], max(int(k), 0)
        vol = np.zeros((n, kk), np.int32)
        dist = np.zeros((n, kk), np.float32)
        cnt = np.zeros(n, np.int32)
        check(lib().rt_sarsa_knn(self.ctx.handle, self._h, _fp(p), _fp(n_), n, int(k),
                                 self.knn_reach() if radius is None else float(radius), _ip(vol), _fp(dist), _ip(cnt)))
        return vol, dist, cnt

    def irradiance_view(self, cam, params, k: int = 3, radius: float | None = None, weight: int = RT_IRR_MEAN,
                        tint: bool = True, first_sample: int = 0, aov: bool = False):
        """The irradiance render of the map (draw_radiance_map_path_tracing of the CPU engine;
        rt_render_irradiance): every camera hit as the mean (RT_IRR_MEAN) or cone-weighted mean
        (RT_IRR_CONE) of the irradiance estimates of its k nearest volumes within radius (None: the
        reach), times albedo / luminance with tint.  Returns rgb (H, W, 3); with aov, (rgb, tri,
        pos, vol (H, W, k), dist (H, W, k)) of sample first_sample.  The map is left as it is."""
        h, w = params.height, params.width
        o = self._irr_opts(k, radius, weight, tint)
        out = np.zeros((h, w, 3), np.float32)
        if not aov:
            check(lib().rt_render_irradiance(self.ctx.handle, self.scene.handle, self._h, ctypes.byref(cam),
                                             ctypes.byref(params), ctypes.byref(o), first_sample, _fp(out), None, None,
                                             None, None))
            return out
        kk = max(int(k), 0)
        tri = np.zeros((h, w), np.int32)
        pos = np.zeros((h, w, 3), np.float32)
        vol = np.zeros((h, w, kk), np.int32)
        dist = np.zeros((h, w, kk), np.float32)
        check(lib().rt_render_irradiance(self.ctx.handle, self.scene.handle, self._h, ctypes.byref(cam),
                                         ctypes.byref(params), ctypes.byref(o), first_sample, _fp(out), _ip(tri), _fp(pos),
                                         _ip(vol), _fp(dist)))
        return out, tri, pos, vol, dist

    def irradiance_view_tiles_device(self, cam, params, tiles: np.ndarray, tile_size: int, out_ptr: int, stream: int,
                                     k: int = 3, radius: float | None = None, weight: int = RT_IRR_MEAN,
                                     tint: bool = True, first_sample: int = 0) -> None:
        """irradiance_view over a tile list into device memory, stream-ordered; tiles and output
        layout as render_tiles_device (rt_render_irradiance_tiles_device)."""
        t = np.ascontiguousarray(tiles, np.int32).reshape(-1, 2)
        o = self._irr_opts(k, radius, weight, tint)
        check(lib().rt_render_irradiance_tiles_device(self.ctx.handle, self.scene.handle, self._h, ctypes.byref(cam),
                                                      ctypes.byref(params), ctypes.byref(o), first_sample, _ip(t),
                                                      t.shape[0], tile_size, ctypes.c_void_p(out_ptr),
                                                      ctypes.c_void_p(stream)))

    def td_device(self):
        """Device pointers of the frame's TD sums (int64, fixed point 2^-32) and counts (uint32)."""
        s, c, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(0)
        check(lib().rt_sarsa_td_device(self._h, ctypes.byref(s), ctypes.byref(c), ctypes.byref(n)))
        return int(s.value or 0), int(c.value or 0), int(n.value)

    def apply(self, stream: int = 0) -> None:
        check(lib().rt_sarsa_apply(self._h, ctypes.c_void_p(stream)))

    def close(self):
        if self._h:
            lib().rt_sarsa_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def voronoi_palette(seed: int, n: int) -> np.ndarray:
    """The random per-volume colours of seed `seed`, (n, 3) in [0, 1) (rt_sarsa_voronoi_palette;
    RadianceMap::set_voronoi_colours)."""
    out = np.zeros((max(n, 0), 3), np.float32)
    check(lib().rt_sarsa_voronoi_palette(seed, n, _fp(out)))  # (n < 0: refused there)
    return out


# ---- colour tables for RadianceMap.set_view_colours from RadianceMap.read() ----

def irradiance_colours(irradiance: np.ndarray) -> np.ndarray:
    """The irradiance estimate accumulators as grey, scaled to the largest one."""
    a = np.maximum(np.asarray(irradiance, np.float32), 0)
    top = float(a.max()) if a.size else 0.0
    g = a / np.float32(top) if top > 0 else np.zeros_like(a)
    return np.repeat(g[:, None], 3, axis=1).astype(np.float32)


def visits_colours(visits: np.ndarray) -> np.ndarray:
    """Each volume's visits summed over its sectors, as grey on a log scale."""
    tot = np.asarray(visits, np.uint64).reshape(-1, SECTORS).sum(axis=1).astype(np.float64)
    top = float(tot.max()) if tot.size else 0.0
    g = np.log1p(tot) / np.log1p(top) if top > 0 else np.zeros_like(tot)
    return np.repeat(g[:, None], 3, axis=1).astype(np.float32)


def max_q_colours(q: np.ndarray) -> np.ndarray:
    """The first sector of largest Q (the max-direction sampler's sector) as a colour: sector
    12 x + y -> hue x / 12 at full saturation, value (y + 1) / 12."""
    k = np.argmax(np.asarray(q, np.float32).reshape(-1, SECTORS), axis=1)  # the first maximum
    hue = (k // 12).astype(np.float32) / np.float32(12)
    val = ((k % 12) + 1).astype(np.float32) / np.float32(12)
    h6 = hue * np.float32(6)
    # HSV -> RGB at saturation 1: channel c = value * clip(|((h6 + shift_c) mod 6) - 3| - 1, 0, 1)
    rgb = [np.clip(np.abs(np.mod(h6 + np.float32(s), 6) - 3) - 1, 0, 1) * val for s in (0, 4, 2)]
    return np.stack(rgb, axis=1).astype(np.float32)


def stats_line(path_floor_sum: int, zero_paths: int, pixels: int) -> str:
    """`avg << " " << 0.0 << " " << zero` with ostream defaults: avg = float(int / int)."""
    avg = np.float32(path_floor_sum // pixels)
    return f"{float(avg):g} {0.0:g} {zero_paths}\n"


def read_q_file(path: str):
    """radiance_map_data.txt -> (positions [n, 3], Q [n, 144])."""
    with open(path) as fh:
        actions = int(fh.readline())
        rows = [np.array(l.split(), np.float64) for l in fh if l.strip()]
    a = np.array(rows).reshape(len(rows), 3 + actions)
    return a[:, :3].astype(np.float32), a[:, 3:].astype(np.float32)


def read_q(path: str):
    """radiance_map_data.txt -> (positions [n, 3], Q [n, actions]) through the library's own
    parser (rt_qtable_read, the reference trainer's load_radiance_map_data): every value is
    strtof of its printed token; a malformed file raises RtError naming the line."""
    n, a = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().rt_qtable_read(os.fsencode(path), ctypes.byref(n), ctypes.byref(a), None, None))
    pos = np.zeros((n.value, 3), np.float32)
    q = np.zeros((n.value, a.value), np.float32)
    check(lib().rt_qtable_read(os.fsencode(path), ctypes.byref(n), ctypes.byref(a), _fp(pos), _fp(q)))
    return pos, q


def read_selected_file(path: str):
    """selected_sarsa.txt / selected_deep.txt -> (positions, normals, distributions [n, 144])."""
    with open(path) as fh:
        rows = [np.array(l.split(), np.float64) for l in fh if l.strip()]
    a = np.array(rows).reshape(len(rows), -1)
    return a[:, :3].astype(np.float32), a[:, 3:6].astype(np.float32), a[:, 6:].astype(np.float32)
