"""Radiance-volume glyphs: saved sector distributions drawn inside the scene (rtmi.h
"radiance-volume glyphs"; the reference's RENDER_SAVED_RADIANCE_VOLUMES picture).

  read_selected(path)             selected_sarsa.txt / selected_deep.txt / selected_true.txt ->
                                  (positions, normals, distributions (n, 144))  (rt_selected_read)
  glyph_mesh(pos, nrm, diameter)  the 288 triangles and 144 quad normals of every glyph, host only
  glyph_colours(values, mode)     the sector colours, RATIO (GPU engine) or MAGNITUDE (CPU engine)
  Glyphs(ctx, pos, nrm, values, diameter, colour_mode)   the set on the device, with its BVH
  .view(scene, cam, params, first, base, shade, aov)      the glyphs over a base frame (or the
                                  scene's albedo / emission / env_light), k_glyph_view
  .view_tiles_device(...)         the same over a tile list into device memory
  .set_colours(rgb)               another (n, 144, 3) colour table
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._lib import (RT_GLYPH_MAGNITUDE, RT_GLYPH_MAX, RT_GLYPH_RATIO, RT_GLYPH_SECTORS, RT_GLYPH_TRIS, RtGlyphViewOpts,
                   check, lib)
from .api import Context, Scene, _fp, _ip

RATIO = RT_GLYPH_RATIO          # (ratio, 1 - ratio, 0), ratio = value / the row's largest
MAGNITUDE = RT_GLYPH_MAGNITUDE  # grey 1 - |value| / the row's largest magnitude
SECTORS = RT_GLYPH_SECTORS
TRIS = RT_GLYPH_TRIS
MAX = RT_GLYPH_MAX
DIAMETER = 0.15  # the reference's DIAMETER (it acts as a radius)


def _rows(a, cols) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).reshape(-1, cols)


def read_selected(path: str):
    """A per-volume file of rt_sarsa_save_selected, rt_dqn_save_selected or
    tools/true_distribution.py: (positions (n, 3), normals (n, 3), distributions (n, 144))."""
    n = ctypes.c_int32(0)
    check(lib().rt_selected_read(os.fsencode(path), ctypes.byref(n), None, None, None))
    pos = np.zeros((n.value, 3), np.float32)
    nrm = np.zeros((n.value, 3), np.float32)
    val = np.zeros((n.value, SECTORS), np.float32)
    check(lib().rt_selected_read(os.fsencode(path), ctypes.byref(n), _fp(pos), _fp(nrm), _fp(val)))
    return pos, nrm, val


def glyph_mesh(pos, normal, diameter: float = DIAMETER):
    """(triangles (n, 288, 9), quad normals (n, 144, 3)) of the glyphs at pos with normals
    `normal` (used as given) and radius `diameter` (rt_glyph_mesh)."""
    p, nr = _rows(pos, 3), _rows(normal, 3)
    if p.shape != nr.shape:
        raise ValueError(f"positions {p.shape} and normals {nr.shape} differ")
    n = p.shape[0]
    tri = np.zeros((n, TRIS, 9), np.float32)
    qn = np.zeros((n, SECTORS, 3), np.float32)
    check(lib().rt_glyph_mesh(_fp(p), _fp(nr), n, float(diameter), _fp(tri), _fp(qn)))
    return tri, qn


def glyph_colours(values, mode: int = RATIO) -> np.ndarray:
    """The sector colours (n, 144, 3) of distributions (n, 144) (rt_glyph_colours)."""
    v = _rows(values, SECTORS)
    rgb = np.zeros((v.shape[0], SECTORS, 3), np.float32)
    check(lib().rt_glyph_colours(_fp(v), v.shape[0], int(mode), _fp(rgb)))
    return rgb


class Glyphs:
    """A glyph set on the device (rt_glyphs_create): at most MAX glyphs; none is a valid set.
    diameter: one for all glyphs, or an array of one per glyph (rt_glyphs_create_sized)."""

    def __init__(self, ctx: Context, pos, normal, values, diameter: float = DIAMETER, colour_mode: int = RATIO):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        p, nr, v = _rows(pos, 3), _rows(normal, 3), _rows(values, SECTORS)
        if not (p.shape[0] == nr.shape[0] == v.shape[0]):
            raise ValueError(f"{p.shape[0]} positions, {nr.shape[0]} normals, {v.shape[0]} distributions")
        if np.ndim(diameter) == 0:
            check(lib().rt_glyphs_create(ctx.handle, _fp(p), _fp(nr), _fp(v), p.shape[0], float(diameter),
                                         int(colour_mode), ctypes.byref(self._h)))
        else:  # a diameter per glyph
            d = np.ascontiguousarray(diameter, np.float32).ravel()
            if d.shape[0] != p.shape[0]:
                raise ValueError(f"{p.shape[0]} glyphs, {d.shape[0]} diameters")
            check(lib().rt_glyphs_create_sized(ctx.handle, _fp(p), _fp(nr), _fp(v), _fp(d), p.shape[0], int(colour_mode),
                                               ctypes.byref(self._h)))
        info = self.info()
        self.n_glyphs, self.n_tri = info["glyphs"], info["triangles"]

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        n, t, b = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        check(lib().rt_glyphs_info(self._h, ctypes.byref(n), ctypes.byref(t), ctypes.byref(b)))
        return {"glyphs": int(n.value), "triangles": int(t.value), "bvh_nodes": int(b.value)}

    def set_colours(self, rgb) -> None:
        """The caller's own sector colours, (n_glyphs, 144, 3) (rt_glyphs_set_colours)."""
        t = np.ascontiguousarray(rgb, np.float32)
        if t.shape != (self.n_glyphs, SECTORS, 3):
            raise ValueError(f"colour table must be ({self.n_glyphs}, {SECTORS}, 3), got {t.shape}")
        check(lib().rt_glyphs_set_colours(self._h, _fp(t)))

    def view(self, scene: Scene, cam, params, first: int = 0, base=None, shade: bool = False, aov: bool = False):
        """The glyphs over `base` ((H, W, 3); None: the scene's albedo, its lights' emission and
        env_light), samples first .. first + spp - 1 of the camera rays of RadianceMap.view
        (rt_render_glyph_view).  Returns rgb (H, W, 3); with aov, (rgb, tri, glyph, sector, t) of
        sample `first`: the scene's own hit, the winning glyph and sector (-1: none), the winner's t
        (+inf: a miss)."""
        h, w = params.height, params.width
        out = np.zeros((h, w, 3), np.float32)
        b = None
        if base is not None:
            b = np.ascontiguousarray(base, np.float32)
            if b.shape != (h, w, 3):
                raise ValueError(f"base must be ({h}, {w}, 3), got {b.shape}")
        opts = RtGlyphViewOpts(int(bool(shade)))
        bp = None if b is None else _fp(b)
        if not aov:
            check(lib().rt_render_glyph_view(self.ctx.handle, scene.handle, self._h, ctypes.byref(cam), ctypes.byref(params),
                                             ctypes.byref(opts), first, bp, _fp(out), None, None, None, None))
            return out
        tri = np.zeros((h, w), np.int32)
        gl = np.zeros((h, w), np.int32)
        sec = np.zeros((h, w), np.int32)
        t = np.zeros((h, w), np.float32)
        check(lib().rt_render_glyph_view(self.ctx.handle, scene.handle, self._h, ctypes.byref(cam), ctypes.byref(params),
                                         ctypes.byref(opts), first, bp, _fp(out), _ip(tri), _ip(gl), _ip(sec), _fp(t)))
        return out, tri, gl, sec, t

    def view_tiles_device(self, scene: Scene, cam, params, tiles: np.ndarray, tile_size: int, out_ptr: int, stream: int,
                          first: int = 0, base_ptr: int = 0, shade: bool = False) -> None:
        """The view over a tile list into device memory, stream-ordered; tiles and output layout as
        render_tiles_device; base_ptr: the whole W x H x 3 base image on the device, or 0
        (rt_render_glyph_view_tiles_device)."""
        t = np.ascontiguousarray(tiles, np.int32).reshape(-1, 2)
        opts = RtGlyphViewOpts(int(bool(shade)))
        check(lib().rt_render_glyph_view_tiles_device(self.ctx.handle, scene.handle, self._h, ctypes.byref(cam),
                                                      ctypes.byref(params), ctypes.byref(opts), first,
                                                      ctypes.c_void_p(base_ptr or None), _ip(t), t.shape[0], tile_size,
                                                      ctypes.c_void_p(out_ptr or None), ctypes.c_void_p(stream or None)))

    def close(self):
        if self._h:
            lib().rt_glyphs_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
