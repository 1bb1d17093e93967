"""Scenes and ray sets shared by the candidate-table tests (test_ctab.py, test_cand_route.py)."""
import os

import numpy as np

from conftest import MODELS


def _scene(rtmi_mod, kind):
    if kind == "cornell_cpu":
        g = rtmi_mod.cornell_geometry(0)
    elif kind == "cornell_gpu":
        g = rtmi_mod.cornell_geometry(1)
    elif kind == "bunny":
        g = rtmi_mod.obj_geometry(os.path.join(MODELS, "bunny.obj"), "generic")
    else:
        g = rtmi_mod.obj_geometry(os.path.join(MODELS, kind + ".obj"), kind)
    return np.ascontiguousarray(g.all_triangles(), np.float32), g.n_surf


def _frame(n):
    t = np.array([n[2], 0.0, -n[0]]) if abs(n[0]) > abs(n[1]) else np.array([0.0, -n[2], n[1]])
    t = t / np.linalg.norm(t)
    return t, np.cross(n, t)


def bounce_rays(tri, n_surf, n, seed):
    """(surf, origin, direction, kind) of n rays leaving random surface points as the kernel
    forms them: o = pos + 1e-5 sd, d = sd / |sd| in float32 (kind 0: uniform hemisphere, 1: at
    a vertex of the scene, 2: nearly parallel to some triangle's plane, 3: nearly parallel to
    the origin's own plane)"""
    rng = np.random.default_rng(seed)
    v = tri[:n_surf].reshape(-1, 3, 3).astype(np.float64)
    N = np.cross(v[:, 2] - v[:, 0], v[:, 1] - v[:, 0])
    area = 0.5 * np.linalg.norm(N, axis=1)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    j = rng.choice(n_surf, n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    f = a + b > 1
    a[f], b[f] = 1 - a[f], 1 - b[f]
    pos = (v[j, 0] + a[:, None] * (v[j, 1] - v[j, 0]) + b[:, None] * (v[j, 2] - v[j, 0])).astype(np.float32)
    allv = tri.reshape(-1, 3).astype(np.float64)
    kind = rng.integers(0, 4, n)
    sd = np.zeros((n, 3))
    for i in range(n):
        nn = N[j[i]]
        if kind[i] == 0:
            T, B = _frame(nn)
            r1, r2 = rng.random(), rng.random()
            st = np.sqrt(max(0.0, 1 - r1 * r1))
            s = st * np.cos(2 * np.pi * r2) * B + r1 * nn + st * np.sin(2 * np.pi * r2) * T
        elif kind[i] == 1:
            s = allv[rng.integers(0, len(allv))] - pos[i] + rng.normal(size=3) * 10.0 ** rng.uniform(-7, -3)
        else:
            k = rng.integers(0, len(tri)) if kind[i] == 2 else j[i]
            vk = tri[k].reshape(3, 3).astype(np.float64)
            nk = np.cross(vk[1] - vk[0], vk[2] - vk[0])
            nk /= np.linalg.norm(nk)
            T, B = _frame(nk)
            ph = 2 * np.pi * rng.random()
            s = np.cos(ph) * T + np.sin(ph) * B + nk * abs(rng.normal()) * 10.0 ** rng.uniform(-7, -1.5)
        if np.dot(s, nn) < 0:
            s = -s
        sd[i] = s / np.linalg.norm(s)
    sd = sd.astype(np.float32)
    o = (pos + np.float32(1e-5) * sd).astype(np.float32)
    ln = np.sqrt((sd[:, 0] * sd[:, 0] + sd[:, 1] * sd[:, 1]) + sd[:, 2] * sd[:, 2]).astype(np.float32)
    d = (sd / ln[:, None]).astype(np.float32)
    return j.astype(np.int32), o, d, kind
