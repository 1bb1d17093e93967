"""Ground-truth incident radiance at surface points (rt_probe_radiance, include/rtmi.h).

The thesis sets the radiance map's and the network's normalised Q values beside "the true
incident radiance distribution" at selected points, "calculated by firing 4096 sampled light
paths per sector and averaging their incident radiance approximation"
(Descriptions/write_up/chapters/4_critical_evaluation.tex:92-110); the reference ships the
picture and no code for it.  radiance() is that estimate on the device, distribution() its
normalised form and distribution_error() the distance of a learned distribution from it.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from ._lib import RtParams, check, lib
from .api import Context, Scene

SECTORS = 144  # RT_PROBE_SECTORS: the sampler's 12 x 12 cells, k = gx * 12 + gy
MAX_ID = (1 << 32) // SECTORS  # ids below it: the Philox pixel word id * 144 + k fits 32 bits


def _fp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def radiance(ctx: Context, scene: Scene, params: RtParams, pos, tri, ids, first_sample: int = 0,
             want_irr: bool = True, want_dir: bool = False) -> dict:
    """rt_probe_radiance on host arrays: pos (n, 3) points on the surfaces tri (n,), ids (n,) the
    points' RNG identities.  Returns {"rad": (n, 144, 3) mean incoming radiance per sector,
    "irr": the same weighted by the cosine to the normal (want_irr), "dir": the first direction of
    sample first_sample (want_dir), "casts": closest-hit calls}.  A point's result depends on the
    scene, params, its own pos / tri / id and first_sample alone, bit for bit."""
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tri, np.int32).ravel()
    i = np.ascontiguousarray(ids, np.uint32).ravel()
    n = p.shape[0]
    if t.shape[0] != n or i.shape[0] != n:
        raise ValueError("pos, tri and ids: one entry per point")
    rad = np.zeros((n, SECTORS, 3), np.float32)
    irr = np.zeros((n, SECTORS, 3), np.float32) if want_irr else None
    dr = np.zeros((n, SECTORS, 3), np.float32) if want_dir else None
    casts = ctypes.c_uint64(0)
    check(lib().rt_probe_radiance(ctx.handle, scene.handle, ctypes.byref(params), _fp(p),
                                  t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                  i.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n, int(first_sample),
                                  _fp(rad), _fp(irr), _fp(dr), ctypes.byref(casts)))
    out = {"rad": rad, "casts": int(casts.value)}
    if want_irr:
        out["irr"] = irr
    if want_dir:
        out["dir"] = dr
    return out


def radiance_device(ctx: Context, scene: Scene, params: RtParams, pos_ptr: int, tri_ptr: int, ids_ptr: int, n: int,
                    first_sample: int, rad_ptr: int, irr_ptr: int = 0, dir_ptr: int = 0, casts_ptr: int = 0,
                    stream: int = 0) -> None:
    """rt_probe_radiance_device: the same on device pointers (0 = NULL for the optional ones),
    asynchronous on `stream`; the uint64 at casts_ptr is accumulated into.  tri and ids are not
    checked on the host: a point that radiance() would refuse gets zeros."""
    vp = ctypes.c_void_p
    check(lib().rt_probe_radiance_device(ctx.handle, scene.handle, ctypes.byref(params), vp(pos_ptr), vp(tri_ptr),
                                         vp(ids_ptr), int(n), int(first_sample), vp(rad_ptr), vp(irr_ptr or None),
                                         vp(dir_ptr or None), vp(casts_ptr or None), vp(stream)))


def distribution(rad) -> np.ndarray:
    """The normalised luminance per sector, (r + g + b) / 3 divided by its sum over the 144
    sectors, in float64: the form of selected_sarsa.txt's d0 .. d143.  rad: (..., 144, 3).  A
    point that received no radiance at all has no distribution: its row is all zeros."""
    r = np.asarray(rad, np.float64)
    if r.shape[-2:] != (SECTORS, 3):
        raise ValueError(f"rad must end in ({SECTORS}, 3), got {r.shape}")
    lum = r.sum(axis=-1) / 3.0
    tot = lum.sum(axis=-1, keepdims=True)
    return np.divide(lum, tot, out=np.zeros_like(lum), where=tot > 0.0)


def distribution_error(true, learned) -> dict:
    """Per point, the distance of a learned sector distribution from the true one, both
    (..., 144) and non-negative; each is divided by its own sum first (a Q row need not be
    normalised).  {"tv": total variation 0.5 * sum |p - q| in [0, 1], "kl": KL(p || q) =
    sum p log(p / q) in nats}.
    Zeros: a sector with p = 0 adds nothing to the KL sum (the limit of x log x); a sector with
    p > 0 and q = 0 makes it +inf (the learned distribution never samples a direction that
    carries light); a row whose p or q sums to 0 is no distribution: both figures are nan."""
    p = np.asarray(true, np.float64)
    q = np.asarray(learned, np.float64)
    if p.shape != q.shape or p.shape[-1] != SECTORS:
        raise ValueError(f"true and learned must share a shape ending in {SECTORS}")
    if (p < 0).any() or (q < 0).any():
        raise ValueError("distributions must be non-negative")
    sp, sq = p.sum(axis=-1, keepdims=True), q.sum(axis=-1, keepdims=True)
    ok = ((sp > 0) & (sq > 0))[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        pn, qn = p / sp, q / sq
        tv = 0.5 * np.abs(pn - qn).sum(axis=-1)
        term = np.where(pn > 0, pn * (np.log(pn) - np.log(qn)), 0.0)
        kl = term.sum(axis=-1)
    nan = np.full(ok.shape, np.nan)
    return {"tv": np.where(ok, tv, nan), "kl": np.where(ok, kl, nan)}


def write_selected_file(path: str, pos, nrm, dist) -> None:
    """selected_true.txt, in the format of selected_sarsa.txt / selected_deep.txt (one line per
    point: "x y z nx ny nz d0 .. d143", ostream defaults: 6 significant digits); sarsa.
    read_selected_file reads it back."""
    p = np.asarray(pos, np.float64).reshape(-1, 3)
    nn = np.asarray(nrm, np.float64).reshape(-1, 3)
    d = np.asarray(dist, np.float64).reshape(-1, SECTORS)
    if not (p.shape[0] == nn.shape[0] == d.shape[0]):
        raise ValueError("pos, nrm and dist: one row per point")
    with open(path, "w") as fh:
        for a, b, c in zip(p, nn, d):
            fh.write(" ".join(f"{float(v):g}" for v in (*a, *b, *c)) + "\n")
