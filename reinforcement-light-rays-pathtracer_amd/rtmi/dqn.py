"""DQN Q-value network (BASELINE config 4) on top of the C ABI.

  read_dynet(path)        the reference's DyNet text models (Radiance_Map_Data/*.model),
                          via rt_dynet_read; W row-major [out][in]
  write_dynet(path, params)   the same format out (rt_dynet_write), e.g. DqnTrainer.params()
  synthetic_weights(...)  seeded He-normal weights for scenes whose trained model the
                          reference does not ship (archway: 918 inputs)
  exact_weights / selection_weights / grid_points   networks and rays on which the bf16
                          forward is exact, so the device's Q can be pinned bit for bit
  Dqn(ctx, nn_vertices, weights)   device network (rt_dqn_create)
  forward / sample / render / render_tiles_device
  Dqn.set_sampling(SAMPLE_MAX)   the reference's sample_max_direction in render / render_tiles_device
                          (rt_dqn_set_sampling); sample_max the sampler alone; enable_stats(ctx) then
                          render_stats(ctx) the last render's (paths, zero-contribution paths)
  render_view / render_view_tiles_device   the Q-network view (rt_render_dqn_view): the network's
                          irradiance estimate at every camera hit, on rt_render_irradiance's scale
  DqnTrainer(ctx, nn_vertices, weights)   Neural-Q training (rt_dqn_trainer_*): TD targets,
                          one Adam step per batch, parameters out for a new Dqn; forward_device
                          its own fp32 forward (read-only)
  NeuralQ(ctx, scene, trainer)    the renderer that trains while it renders (rt_neuralq_*);
                          read_rays() the per-ray arrays of the last frame
  QFit(ctx, trainer, pos, q) / QFit.from_map / QFit.from_file   the reference's NN_Q_Value_Trainer:
                          the network fitted to a radiance map's Q-table (rt_dqn_fit_*), epoch()
                          -> (loss, test error); fit_order(seed, n) its split and shuffle;
                          DqnTrainer.fit_step_device / fit_error_device one dense step / the error
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import RT_DQN_SAMPLE_CDF, RT_DQN_SAMPLE_MAX, RT_DQN_VIEW_IRRADIANCE, RtDqnViewOpts, check, lib
from .api import Context, Scene, _fp, _ip

HIDDEN = (200, 300, 200)  # NN_Builders/dq_network.cu:14-17
ACTIONS = 144             # GRID_RESOLUTION^2
SAMPLE_CDF = RT_DQN_SAMPLE_CDF   # importance_sample_direction (default)
SAMPLE_MAX = RT_DQN_SAMPLE_MAX   # sample_max_direction: the first cell of the largest positive Q


def read_dynet(path: str) -> List[np.ndarray]:
    """Parameters of a DyNet TextFileSaver model in file order (row-major)."""
    L = lib()
    n_params, n_values = ctypes.c_int(0), ctypes.c_int64(0)
    check(L.rt_dynet_read(path.encode(), 0, None, None, None, ctypes.byref(n_params),
                          ctypes.byref(n_values)))
    rows = np.zeros(n_params.value, np.int32)
    cols = np.zeros(n_params.value, np.int32)
    vals = np.zeros(n_values.value, np.float32)
    check(L.rt_dynet_read(path.encode(), n_params.value, _ip(rows), _ip(cols), _fp(vals),
                          ctypes.byref(n_params), ctypes.byref(n_values)))
    out, off = [], 0
    for r, c in zip(rows, cols):  # cols 0: a vector ("{rows}" header)
        n = int(r) * max(int(c), 1)
        a = vals[off:off + n]
        out.append(a.copy() if c == 0 else a.reshape(int(r), int(c)).copy())
        off += n
    return out


def write_dynet(path: str, params: Sequence[np.ndarray]) -> None:
    """DyNet TextFileSaver model (neural_q_pathtracer.cu:193) of `params` in order: matrices
    row-major [rows][cols], vectors [rows]; read_dynet(path) returns them bit for bit, shapes
    included (an (n, 1) matrix stays one).  Non-finite values raise (DyNet cannot load them)."""
    arrs = [np.ascontiguousarray(p, np.float32) for p in params]
    for a in arrs:
        if a.ndim not in (1, 2) or a.size == 0:
            raise ValueError(f"DyNet parameters are non-empty vectors or matrices, got {a.shape}")
    rows = np.array([a.shape[0] for a in arrs], np.int32)
    cols = np.array([a.shape[1] if a.ndim == 2 else 0 for a in arrs], np.int32)  # 0: vector
    vals = np.concatenate([a.ravel() for a in arrs]) if arrs else np.zeros(1, np.float32)
    check(lib().rt_dynet_write(os.fsencode(path), len(arrs), _ip(rows), _ip(cols), _fp(vals)))


def join_layers(W: Sequence[np.ndarray], b: Sequence[np.ndarray]) -> list:
    """([W1..W4], [b1..b4]) -> [W1, b1, ..., W4, b4] (the reference's parameter order)"""
    return [x for pair in zip(W, b) for x in pair]


def split_layers(params: Sequence[np.ndarray]) -> Tuple[list, list]:
    """[W1, b1, ..., W4, b4] -> ([W1..W4], [b1..b4])"""
    if len(params) != 8:
        raise ValueError(f"expected 8 parameters (4 affine layers), got {len(params)}")
    return [np.ascontiguousarray(params[i], np.float32) for i in (0, 2, 4, 6)], \
           [np.ascontiguousarray(params[i], np.float32).ravel() for i in (1, 3, 5, 7)]


def synthetic_weights(n_in: int, seed: int = 1984, hidden=HIDDEN, n_out: int = ACTIONS,
                      bias: float = 0.05) -> Tuple[list, list]:
    """He-normal (std sqrt(2/fan_in)) weights from numpy's PCG64 seeded with `seed`, constant
    positive biases: a stand-in for models the reference does not ship."""
    rng = np.random.default_rng(seed)
    dims = [n_in, *hidden, n_out]
    W = [(rng.standard_normal((dims[i + 1], dims[i])) * np.sqrt(2.0 / dims[i])).astype(np.float32)
         for i in range(4)]
    b = [np.full(dims[i + 1], bias, np.float32) for i in range(4)]
    return W, b


def glorot_weights(n_in: int, seed: int = 1984, hidden=HIDDEN, n_out: int = ACTIONS) -> Tuple[list, list]:
    """DyNet's default initialiser, the one the reference's network starts from (FCLayer's
    model.add_parameters with no initializer, NN_Builders/fc_layer.cu:32-33: ParameterInitGlorot,
    gain 1): uniform in +-sqrt(6 / sum of the tensor's dims) -- sqrt(6 / (out + in)) for a weight
    matrix, sqrt(6 / out) for a bias -- here from numpy's PCG64 seeded with `seed` (DyNet's own
    random stream is not reproducible without DyNet)."""
    rng = np.random.default_rng(seed)
    dims = [n_in, *hidden, n_out]
    W, b = [], []
    for i in range(4):
        sw = np.sqrt(6.0 / (dims[i + 1] + dims[i]))
        W.append(rng.uniform(-sw, sw, (dims[i + 1], dims[i])).astype(np.float32))
        sb = np.sqrt(6.0 / dims[i + 1])
        b.append(rng.uniform(-sb, sb, dims[i + 1]).astype(np.float32))
    return W, b


# ---- networks on which the bf16 forward is exact (tests/test_dqn_forward_exact.py) ----
# Integer weights and biases with every coordinate on the grid of eighths: every product and
# partial sum of every layer is a multiple of EXACT_GRID, bf16 rounding keeps it one, and
# while sum |w a| + |b| <= 2^24 * EXACT_GRID the fp32 accumulation is exact in any order, so
# the device's Q equals the fp64-accumulating restatement's bit for bit.
EXACT_GRID = 0.125
EXACT_HALF = 32            # grid points per axis on each side of 0: coordinates in [-4, 4]
EXACT_FILLS = ("dense", "sparse")


def mlp_rows() -> int:
    """rays per workgroup of the weight-streaming forward kernel in this build (rt_dqn_mlp_rows)"""
    return int(lib().rt_dqn_mlp_rows())


def grid_points(n: int, seed: int = 1984) -> np.ndarray:
    """n points of the 65^3 grid of eighths in [-4, 4]^3 in a seeded order, distinct while
    n <= 65^3 (the order wraps after that); the first m rows of grid_points(n) are
    grid_points(m)."""
    side = 2 * EXACT_HALF + 1
    idx = np.resize(np.random.default_rng(seed).permutation(side ** 3), n)
    ijk = np.stack([idx // (side * side), (idx // side) % side, idx % side], axis=1)
    return ((ijk - EXACT_HALF) * EXACT_GRID).astype(np.float32)


def exact_weights(n_in: int, hidden=HIDDEN, fill: str = "dense", seed: int = 1984,
                  n_out: int = ACTIONS) -> Tuple[list, list, np.ndarray]:
    """(W, b, nn_vertices) of an integer network: layer 0 from {-1, 0, 1} with 8 non-zeros per
    row; layers 1-3 from {-1, +1} with every entry non-zero (`dense`), or 12 non-zeros per
    row from {-2, -1, 1, 2} (`sparse`); biases non-zero integers in [-3, 3]; nn_vertices on the grid
    of eighths in [-4, 4].  A row of a hidden layer with no positive weight is negated, so a
    narrow layer (one feature) still passes its input on."""
    if fill not in EXACT_FILLS:
        raise ValueError(f"fill must be one of {EXACT_FILLS}, got {fill!r}")
    rng = np.random.default_rng(seed)
    dims = [n_in, *hidden, n_out]
    verts = (rng.integers(-EXACT_HALF, EXACT_HALF + 1, n_in) * EXACT_GRID).astype(np.float32)

    def rows(n_rows, n_cols, nnz, values):
        w = np.zeros((n_rows, n_cols), np.float32)
        for o in range(n_rows):
            cols = rng.permutation(n_cols)[:nnz]
            w[o, cols] = rng.choice(values, cols.size)
        return w

    W = [rows(dims[1], n_in, 8, (-1.0, 1.0))]
    for l in range(1, 4):
        if fill == "dense":
            w = rng.choice(np.array((-1.0, 1.0), np.float32), (dims[l + 1], dims[l]))
        else:
            w = rows(dims[l + 1], dims[l], 12, (-2.0, -1.0, 1.0, 2.0))
        if l < 3:
            w[(w <= 0).all(axis=1)] *= -1.0
        W.append(np.ascontiguousarray(w, np.float32))
    b = [rng.choice(np.array((-3, -2, -1, 1, 2, 3), np.float32), dims[l + 1]) for l in range(4)]
    return W, b, verts


def selection_weights(W0: np.ndarray, b0: np.ndarray, sel: Sequence[int], hidden=HIDDEN,
                      n_out: int = ACTIONS) -> Tuple[list, list]:
    """(W, b) with the given layer 0 and 0/1 selection matrices with zero bias behind it, so
    that Q[a] = h1[sel[a]] exactly (a one-term sum; re-rounding a bf16 value changes nothing):
    the folded layer 0 alone, on any input.  hidden[0] is W0's height; with hidden[1] and
    hidden[2] at least that, layers 1-2 pass h1 on and layer 3 selects; otherwise layer 1
    selects (hidden[1], hidden[2] >= n_out) and layers 2-3 pass the selection on."""
    W0 = np.ascontiguousarray(W0, np.float32)
    sel = np.asarray(sel, np.int64)
    h1 = W0.shape[0]
    if hidden[0] != h1 or sel.shape != (n_out,) or sel.min() < 0 or sel.max() >= h1:
        raise ValueError("selection_weights: hidden[0] must be W0's height and sel index it")
    dims = [W0.shape[1], *hidden, n_out]
    W = [W0] + [np.zeros((dims[l + 1], dims[l]), np.float32) for l in range(1, 4)]
    a = np.arange(n_out)
    if hidden[1] >= h1 and hidden[2] >= h1:
        W[1][np.arange(h1), np.arange(h1)] = 1.0
        W[2][np.arange(h1), np.arange(h1)] = 1.0
        W[3][a, sel] = 1.0
    elif hidden[1] >= n_out and hidden[2] >= n_out:
        W[1][a, sel] = 1.0
        W[2][a, a] = 1.0
        W[3][a, a] = 1.0
    else:
        raise ValueError(f"selection_weights: hidden {tuple(hidden)} too narrow")
    b = [np.ascontiguousarray(b0, np.float32).ravel()] + [np.zeros(dims[l + 1], np.float32) for l in range(1, 4)]
    return W, b


class Dqn:
    def __init__(self, ctx: Context, nn_vertices: np.ndarray, W: Sequence[np.ndarray],
                 b: Sequence[np.ndarray]):
        self.ctx = ctx
        self.nn_vertices = np.ascontiguousarray(nn_vertices, np.float32).ravel()
        self.W = [np.ascontiguousarray(w, np.float32) for w in W]
        self.b = [np.ascontiguousarray(x, np.float32).ravel() for x in b]
        self.n_in = int(self.W[0].shape[1])
        if self.nn_vertices.size != self.n_in:
            raise ValueError(f"network has {self.n_in} inputs, scene has {self.nn_vertices.size}")
        hidden = np.array([w.shape[0] for w in self.W[:3]], np.int32)
        Wp = (ctypes.POINTER(ctypes.c_float) * 4)(*[_fp(w) for w in self.W])
        bp = (ctypes.POINTER(ctypes.c_float) * 4)(*[_fp(x) for x in self.b])
        self._h = ctypes.c_void_p()
        check(lib().rt_dqn_create(ctx.handle, _fp(self.nn_vertices), self.n_in, _ip(hidden),
                                  int(self.W[3].shape[0]), Wp, bp, ctypes.byref(self._h)))

    @property
    def handle(self):
        return self._h

    MLP_AUTO, MLP_STREAM, MLP_STATIONARY = 0, 1, 2  # RT_DQN_MLP_*

    def set_mlp(self, mode: int) -> None:
        """forward kernel: MLP_AUTO / MLP_STREAM (weight streaming) or MLP_STATIONARY"""
        check(lib().rt_dqn_set_mlp(self._h, mode))

    SAMPLE_CDF, SAMPLE_MAX = RT_DQN_SAMPLE_CDF, RT_DQN_SAMPLE_MAX

    def set_sampling(self, mode: int) -> None:
        """direction sampling of render / render_tiles_device with this network: SAMPLE_CDF
        (default) or SAMPLE_MAX, the reference's sample_max_direction (rt_dqn_set_sampling)"""
        check(lib().rt_dqn_set_sampling(self._h, mode))

    @property
    def sampling(self) -> int:
        m = ctypes.c_int(0)
        check(lib().rt_dqn_get_sampling(self._h, ctypes.byref(m)))
        return int(m.value)

    def forward(self, loc: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(loc, np.float32).reshape(-1, 3)
        q = np.zeros((x.shape[0], ACTIONS), np.float32)
        check(lib().rt_dqn_forward(self.ctx.handle, self._h, _fp(x), x.shape[0], _fp(q)))
        return q

    def forward_device(self, loc_ptr: int, n: int, q_ptr: int, stream: int = 0) -> None:
        check(lib().rt_dqn_forward_device(self.ctx.handle, self._h, ctypes.c_void_p(loc_ptr), n,
                                          ctypes.c_void_p(q_ptr), ctypes.c_void_p(stream)))

    def save_selected(self, to_select: str, out: str) -> None:
        """selected_deep.txt format for the locations of to_select.txt (rt_dqn_save_selected)."""
        check(lib().rt_dqn_save_selected(self.ctx.handle, self._h, os.fsencode(to_select), os.fsencode(out)))

    def flops_per_ray(self) -> int:
        """2 * sum(in*out) of the four layers (unpadded)"""
        return int(2 * sum(w.shape[0] * w.shape[1] for w in self.W))

    def mfma_flops_per_ray(self) -> int:
        """2 * sum(in*out) of layers 1-3, the ones executed on MFMA (unpadded); layer 0 is
        folded to a 3-input affine map on the VALU (rt_internal.hpp DqnNet)"""
        return int(2 * sum(w.shape[0] * w.shape[1] for w in self.W[1:]))

    def close(self):
        if self._h:
            lib().rt_dqn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sample(ctx: Context, scene: Scene, seed: int, q: np.ndarray, loc: np.ndarray, tri: np.ndarray,
           pix: np.ndarray, sample_idx: int, bounce: int, tp: np.ndarray):
    """Importance-sample directions from Q (rt_dqn_sample).  Returns (q*cos, tp, dir, action)."""
    q = np.ascontiguousarray(q, np.float32).copy()
    loc = np.ascontiguousarray(loc, np.float32)
    tri = np.ascontiguousarray(tri, np.int32)
    pix = np.ascontiguousarray(pix, np.uint32)
    tp = np.ascontiguousarray(tp, np.float32).copy()
    n = q.shape[0]
    d = np.zeros((n, 3), np.float32)
    a = np.zeros(n, np.int32)
    check(lib().rt_dqn_sample(ctx.handle, scene.handle, seed, _fp(q), _fp(loc), _ip(tri),
                              pix.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n, sample_idx,
                              bounce, _fp(tp), _fp(d), _ip(a)))
    return q, tp, d, a


def sample_max(ctx: Context, scene: Scene, seed: int, q: np.ndarray, loc: np.ndarray, tri: np.ndarray,
               pix: np.ndarray, sample_idx: int, bounce: int, tp: np.ndarray):
    """SAMPLE_MAX's sampler alone (rt_dqn_sample_max): the first cell of the largest positive Q
    (0 if none), its jittered direction, tp * cos / (RHO * 2).  q is not modified.  Returns
    (tp, dir, action)."""
    q = np.ascontiguousarray(q, np.float32)
    loc = np.ascontiguousarray(loc, np.float32)
    tri = np.ascontiguousarray(tri, np.int32)
    pix = np.ascontiguousarray(pix, np.uint32)
    tp = np.ascontiguousarray(tp, np.float32).copy()
    n = q.shape[0]
    d = np.zeros((n, 3), np.float32)
    a = np.zeros(n, np.int32)
    check(lib().rt_dqn_sample_max(ctx.handle, scene.handle, seed, _fp(q), _fp(loc), _ip(tri),
                                  pix.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n, sample_idx,
                                  bounce, _fp(tp), _fp(d), _ip(a)))
    return tp, d, a


def enable_stats(ctx: Context, on: bool = True) -> None:
    """count the zero-contribution paths of the renders on ctx from now on (rt_dqn_enable_stats;
    default off: one small kernel per pass)"""
    check(lib().rt_dqn_enable_stats(ctx.handle, int(bool(on))))


def render_stats(ctx: Context) -> Tuple[int, int]:
    """(paths, zero_paths) of the last render / render_tiles_device on ctx (rt_dqn_render_stats):
    the call's valid rays, and those whose final throughput has every channel < 1e-4.  A blocking
    copy (synchronise the stream of a tile render first); raises unless that render ran after
    enable_stats(ctx)."""
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(lib().rt_dqn_render_stats(ctx.handle, ctypes.byref(a), ctypes.byref(b)))
    return int(a.value), int(b.value)


def render(ctx: Context, scene: Scene, dqn: Dqn, cam, params, rect=None):
    x0, y0, w, h = rect if rect is not None else (0, 0, params.width, params.height)
    out = np.zeros((h, w, 3), np.float32)
    casts = ctypes.c_uint64(0)
    check(lib().rt_render_dqn(ctx.handle, scene.handle, dqn.handle, ctypes.byref(cam),
                              ctypes.byref(params), x0, y0, w, h, _fp(out), ctypes.byref(casts)))
    return out, int(casts.value)


def render_tiles_device(ctx: Context, scene: Scene, dqn: Dqn, cam, params, tiles: np.ndarray,
                        tile_size: int, out_ptr: int, casts_ptr: int, stream: int) -> None:
    t = np.ascontiguousarray(tiles, np.int32).reshape(-1, 2)
    check(lib().rt_render_dqn_tiles_device(ctx.handle, scene.handle, dqn.handle, ctypes.byref(cam),
                                           ctypes.byref(params), _ip(t), t.shape[0], tile_size,
                                           ctypes.c_void_p(out_ptr), ctypes.c_void_p(casts_ptr),
                                           ctypes.c_void_p(stream)))


VIEW_OUTPUTS = ("tri", "pos", "q", "action")


def render_view(ctx: Context, scene: Scene, dqn: Dqn, cam, params, tint: bool = False, first_sample: int = 0,
                outputs: Sequence[str] = (), mode: int = RT_DQN_VIEW_IRRADIANCE):
    """The Q-network view (rt_render_dqn_view): per camera hit the network's irradiance estimate
    L = (sum_k Q_k c_k) * luminance / pi * (2 pi / 144) on the cell-centre cosines c_k -- the scale
    of RadianceMap.irradiance_view(k=1) -- grey, or (tint) times albedo / luminance; a light gives
    its emission, a miss env_light.  Returns the image (H, W, 3), or (image, aov) when `outputs`
    names any of VIEW_OUTPUTS: aov["tri"] (H, W) -1 miss / >= n_surf light, aov["pos"] (H, W, 3),
    aov["q"] (H, W, 144) the fp32 forward at the hit point, aov["action"] (H, W) the first cell of
    largest Q_k c_k (-1 without a surface hit), all of sample first_sample."""
    unknown = set(outputs) - set(VIEW_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown view outputs {sorted(unknown)}; choose from {VIEW_OUTPUTS}")
    h, w = params.height, params.width
    out = np.zeros((h, w, 3), np.float32)
    shapes = {"tri": ((h, w), np.int32), "pos": ((h, w, 3), np.float32), "q": ((h, w, ACTIONS), np.float32),
              "action": ((h, w), np.int32)}
    aov = {k: np.zeros(*shapes[k]) for k in VIEW_OUTPUTS if k in outputs}
    opts = RtDqnViewOpts(int(mode), int(bool(tint)))
    check(lib().rt_render_dqn_view(ctx.handle, scene.handle, dqn.handle, ctypes.byref(cam), ctypes.byref(params),
                                   ctypes.byref(opts), int(first_sample), _fp(out),
                                   _ip(aov["tri"]) if "tri" in aov else None,
                                   _fp(aov["pos"]) if "pos" in aov else None,
                                   _fp(aov["q"]) if "q" in aov else None,
                                   _ip(aov["action"]) if "action" in aov else None))
    return (out, aov) if outputs else out


def render_view_tiles_device(ctx: Context, scene: Scene, dqn: Dqn, cam, params, tiles: np.ndarray, tile_size: int,
                             out_ptr: int, stream: int, tint: bool = False, first_sample: int = 0,
                             mode: int = RT_DQN_VIEW_IRRADIANCE) -> None:
    """render_view over a tile list into device memory, stream-ordered; tiles and output layout
    as render_tiles_device (rt_render_dqn_view_tiles_device)."""
    t = np.ascontiguousarray(tiles, np.int32).reshape(-1, 2)
    opts = RtDqnViewOpts(int(mode), int(bool(tint)))
    check(lib().rt_render_dqn_view_tiles_device(ctx.handle, scene.handle, dqn.handle, ctypes.byref(cam),
                                                ctypes.byref(params), ctypes.byref(opts), int(first_sample),
                                                _ip(t), t.shape[0], tile_size, ctypes.c_void_p(out_ptr),
                                                ctypes.c_void_p(stream)))


class DqnTrainer:
    """The Neural-Q learning rule (neural_q_pathtracer.cu:420-513) on the device: fp32
    parameters + DyNet-default Adam (rt_dqn_trainer_create).  Batches are device pointers
    (e.g. torch tensors' data_ptr())."""

    def __init__(self, ctx: Context, nn_vertices: np.ndarray, W: Sequence[np.ndarray],
                 b: Sequence[np.ndarray], learning_rate: float = 1e-3):
        self.ctx = ctx
        self.nn_vertices = np.ascontiguousarray(nn_vertices, np.float32).ravel()
        W = [np.ascontiguousarray(w, np.float32) for w in W]
        b = [np.ascontiguousarray(x, np.float32).ravel() for x in b]
        self.shapes = [w.shape for w in W]
        hidden = np.array([w.shape[0] for w in W[:3]], np.int32)
        Wp = (ctypes.POINTER(ctypes.c_float) * 4)(*[_fp(w) for w in W])
        bp = (ctypes.POINTER(ctypes.c_float) * 4)(*[_fp(x) for x in b])
        self._h = ctypes.c_void_p()
        check(lib().rt_dqn_trainer_create(ctx.handle, _fp(self.nn_vertices), int(W[0].shape[1]), _ip(hidden),
                                          int(W[3].shape[0]), Wp, bp, float(learning_rate),
                                          ctypes.byref(self._h)))

    def close(self) -> None:
        if self._h:
            lib().rt_dqn_trainer_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step_device(self, loc_ptr: int, action_ptr: int, target_ptr: int, n: int,
                    stream: int = 0, sync: bool = True) -> Optional[Tuple[float, float]]:
        """One Adam step; returns (loss, gradient L2 norm before clipping), which waits for
        the stream; sync=False leaves the step in flight and returns None."""
        loss, gn = ctypes.c_float(0.0), ctypes.c_float(0.0)
        check(lib().rt_dqn_train_step_device(self.ctx.handle, self._h, ctypes.c_void_p(loc_ptr),
                                             ctypes.c_void_p(action_ptr), ctypes.c_void_p(target_ptr), n,
                                             ctypes.byref(loss) if sync else None,
                                             ctypes.byref(gn) if sync else None, ctypes.c_void_p(stream)))
        return (float(loss.value), float(gn.value)) if sync else None

    def forward_device(self, loc_ptr: int, n: int, q_ptr: int, stream: int = 0) -> None:
        """Q (n x n_out, device) of n device positions from the current parameters: the fp32
        forward of the training step and of NeuralQ's frame (rt_dqn_trainer_forward_device);
        changes nothing in the trainer; asynchronous on `stream`."""
        check(lib().rt_dqn_trainer_forward_device(self.ctx.handle, self._h, ctypes.c_void_p(loc_ptr), n,
                                                  ctypes.c_void_p(q_ptr), ctypes.c_void_p(stream)))

    def fit_step_device(self, loc_ptr: int, target_ptr: int, n: int, stream: int = 0,
                        sync: bool = True) -> Optional[Tuple[float, float]]:
        """One Adam step of the supervised fit (rt_dqn_fit_step_device): targets n x n_out, the
        squared distance over every output.  Returns and waits as step_device does."""
        loss, gn = ctypes.c_float(0.0), ctypes.c_float(0.0)
        check(lib().rt_dqn_fit_step_device(self.ctx.handle, self._h, ctypes.c_void_p(loc_ptr),
                                           ctypes.c_void_p(target_ptr), n,
                                           ctypes.byref(loss) if sync else None,
                                           ctypes.byref(gn) if sync else None, ctypes.c_void_p(stream)))
        return (float(loss.value), float(gn.value)) if sync else None

    def fit_loss_device(self, q_ptr: int, target_ptr: int, n: int, dq_ptr: int, stream: int = 0,
                        sync: bool = True) -> Optional[float]:
        """The dense loss and its output gradient alone, on device arrays n x n_out
        (rt_dqn_fit_loss_device); sync=False leaves the kernel in flight and returns None."""
        loss = ctypes.c_float(0.0)
        check(lib().rt_dqn_fit_loss_device(self.ctx.handle, self._h, ctypes.c_void_p(q_ptr),
                                           ctypes.c_void_p(target_ptr), n, ctypes.c_void_p(dq_ptr),
                                           ctypes.byref(loss) if sync else None, ctypes.c_void_p(stream)))
        return float(loss.value) if sync else None

    def fit_error_device(self, loc_ptr: int, target_ptr: int, n: int, stream: int = 0) -> float:
        """sum_b ||target_b - Q(loc_b)||^2 over n rows in double, no update
        (rt_dqn_fit_error_device); waits for the stream."""
        e = ctypes.c_double(0.0)
        check(lib().rt_dqn_fit_error_device(self.ctx.handle, self._h, ctypes.c_void_p(loc_ptr),
                                            ctypes.c_void_p(target_ptr), n, ctypes.byref(e),
                                            ctypes.c_void_p(stream)))
        return float(e.value)

    def params(self) -> Tuple[list, list]:
        W = [np.zeros(s, np.float32) for s in self.shapes]
        b = [np.zeros(s[0], np.float32) for s in self.shapes]
        Wp = (ctypes.POINTER(ctypes.c_float) * 4)(*[_fp(w) for w in W])
        bp = (ctypes.POINTER(ctypes.c_float) * 4)(*[_fp(x) for x in b])
        check(lib().rt_dqn_trainer_params(self._h, Wp, bp))
        return W, b

    def grads(self) -> Tuple[list, list]:
        """(dW, db) of the last step, as the backward pass wrote them (before the clipping
        scale), in the layout of params(); a blocking copy; raises if no step has run."""
        W = [np.zeros(s, np.float32) for s in self.shapes]
        b = [np.zeros(s[0], np.float32) for s in self.shapes]
        Wp = (ctypes.POINTER(ctypes.c_float) * 4)(*[_fp(w) for w in W])
        bp = (ctypes.POINTER(ctypes.c_float) * 4)(*[_fp(x) for x in b])
        check(lib().rt_dqn_trainer_gradients(self._h, Wp, bp))
        return W, b


class NeuralQ:
    """NeuralQPathtracer (GPU/deep_learning/neural_q_pathtracer.cu:226-600) on the device:
    epsilon-greedy sampling from the network being trained, trace_ray with rewards (light
    luminance x 200), restarts of terminated rays, the learning rule per batch of rays, one
    stats row per sample (rt_neuralq_render_frame).  The reference's run: archway, batch
    4096, epsilon 0.05 (start = min, decay 0.01), 15 frames of SAMPLES_PER_PIXEL samples."""

    def __init__(self, ctx: Context, scene: Scene, trainer: "DqnTrainer", batch_size: int = 4096,
                 epsilon_start: float = 0.05, epsilon_min: float = 0.05, epsilon_decay: float = 0.01):
        self.ctx, self.scene, self.trainer = ctx, scene, trainer
        self._h = ctypes.c_void_p()
        check(lib().rt_neuralq_create(ctx.handle, scene.handle, trainer._h, int(batch_size), float(epsilon_start),
                                      float(epsilon_min), float(epsilon_decay), ctypes.byref(self._h)))

    @property
    def epsilon(self) -> float:
        e = ctypes.c_float(0.0)
        check(lib().rt_neuralq_epsilon(self._h, ctypes.byref(e)))
        return float(e.value)

    def render_frame(self, cam, params):
        """(image H x W x 3, stats spp x 3 [average path length, loss, zero-contribution
        paths] per sample, ray casts)."""
        img = np.zeros((params.height, params.width, 3), np.float32)
        stats = np.zeros((params.spp, 3), np.float32)
        casts = ctypes.c_uint64(0)
        check(lib().rt_neuralq_render_frame(self.ctx.handle, self._h, ctypes.byref(cam), ctypes.byref(params),
                                            _fp(img), _fp(stats), ctypes.byref(casts)))
        return img, stats, int(casts.value)

    RAY_ARRAYS = (("loc", np.float32, 3), ("tp", np.float32, 3), ("total", np.float32, 3), ("tri", np.int32, 1),
                  ("state", np.uint32, 1), ("bounces", np.uint32, 1), ("action", np.int32, 1),
                  ("reward", np.float32, 1), ("discount", np.float32, 1), ("terminal", np.int32, 1))

    def read_rays(self) -> dict:
        """The per-ray arrays as the last frame left them (rt_neuralq_read_rays), by name:
        loc, tp, total (n, 3); tri, state, bounces, action, reward, discount, terminal (n,).
        Raises before the first frame."""
        n = ctypes.c_int32(0)
        none = [None] * len(self.RAY_ARRAYS)
        check(lib().rt_neuralq_read_rays(self._h, *none, ctypes.byref(n)))
        out = {name: np.zeros((n.value, c) if c > 1 else n.value, dt) for name, dt, c in self.RAY_ARRAYS}
        ptr = {np.float32: ctypes.c_float, np.int32: ctypes.c_int32, np.uint32: ctypes.c_uint32}
        args = [out[name].ctypes.data_as(ctypes.POINTER(ptr[dt])) for name, dt, _ in self.RAY_ARRAYS]
        check(lib().rt_neuralq_read_rays(self._h, *args, None))
        return out

    @staticmethod
    def stats_lines(stats) -> str:
        """nn_training_stats.txt lines (neural_q_pathtracer.cu:577-583): `avg_path_length
        << " " << loss << " " << total_zclp` with ostream defaults (6 significant digits)."""
        out = []
        for avg, loss, z in np.asarray(stats, np.float32):
            out.append(f"{float(avg):g} {float(loss):g} {int(z)}\n")
        return "".join(out)

    def close(self) -> None:
        if self._h:
            lib().rt_neuralq_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


FIT_TAG = 0x51466974        # RT_DQN_FIT_TAG: word 3 of fit_order's Philox counter
FIT_ERROR_CHUNK = 4096      # RT_DQN_FIT_ERROR_CHUNK: rows per forward of fit_error_device


def fit_order(seed: int, n: int, train_fraction: float = 0.8) -> Tuple[np.ndarray, int]:
    """(order, n_train) of rt_dqn_fit_order: the seeded train/test split and shuffle of n rows
    (NN_Q_Value_Trainer's random_shuffle + rand() < 0.8); order[:n_train] are the training
    rows, order[n_train:] the test rows."""
    order = np.zeros(max(int(n), 0), np.int32)
    nt = ctypes.c_int32(0)
    check(lib().rt_dqn_fit_order(seed, int(n), float(train_fraction), _ip(order), ctypes.byref(nt)))
    return order, int(nt.value)


class QFit:
    """The reference's NN_Q_Value_Trainer (NN_Q_Value_Trainer/Source/main.cu:118-294) on the
    device: `trainer`'s network fitted to the rows position -> Q values of a radiance map
    (rt_dqn_fit_*).  pos (n, 3) and q (n, n_out) are host arrays; they are uploaded once in
    fit_order(seed, n, train_fraction)'s order.  The trainer is borrowed: it keeps the fitted
    parameters (trainer.params() -> Dqn / write_dynet) and can go on into NeuralQ."""

    def __init__(self, ctx: Context, trainer: "DqnTrainer", pos: np.ndarray, q: np.ndarray, seed: int = 1984,
                 train_fraction: float = 0.8, batch_size: int = 128):
        self.ctx, self.trainer = ctx, trainer
        self._h = ctypes.c_void_p()
        pos = np.ascontiguousarray(pos, np.float32)
        q = np.ascontiguousarray(q, np.float32)
        if pos.ndim != 2 or pos.shape[1] != 3 or q.ndim != 2 or q.shape[0] != pos.shape[0]:
            raise ValueError(f"pos must be (n, 3) and q (n, actions), got {pos.shape} and {q.shape}")
        check(lib().rt_dqn_fit_create(ctx.handle, trainer._h, _fp(pos), _fp(q), pos.shape[0], q.shape[1], seed,
                                      float(train_fraction), int(batch_size), ctypes.byref(self._h)))

    @classmethod
    def from_map(cls, ctx: Context, trainer: "DqnTrainer", radiance_map, **kw) -> "QFit":
        """The fit of a trained rtmi.sarsa.RadianceMap: its volumes' positions and its Q-table as
        they are on the device (rt_sarsa_volumes + rt_sarsa_read), not the 6 digits of save_q."""
        return cls(ctx, trainer, radiance_map.volumes()[0], radiance_map.read()[0], **kw)

    @classmethod
    def from_file(cls, ctx: Context, trainer: "DqnTrainer", path: str, **kw) -> "QFit":
        """The fit of a radiance_map_data.txt (RadianceMap.save_q), the reference's input."""
        from .sarsa import read_q
        return cls(ctx, trainer, *read_q(path), **kw)

    def info(self) -> dict:
        a, b, c, d = (ctypes.c_int32(0) for _ in range(4))
        check(lib().rt_dqn_fit_info(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return {"n_train": a.value, "n_test": b.value, "n_batches": c.value, "epochs_done": d.value}

    def epoch(self, stream: int = 0) -> Tuple[float, float]:
        """One pass over the training rows and the test error after it: the reference's printed
        (Loss, Error) of an epoch (rt_dqn_fit_epoch); waits once, at the end."""
        loss, e = ctypes.c_double(0.0), ctypes.c_double(0.0)
        check(lib().rt_dqn_fit_epoch(self.ctx.handle, self._h, ctypes.byref(loss), ctypes.byref(e),
                                     ctypes.c_void_p(stream)))
        return float(loss.value), float(e.value)

    @staticmethod
    def epoch_block(i: int, loss: float, error: float) -> str:
        """the reference's per-epoch print (main.cu:279-283; ostream defaults, the sums as the
        floats the reference holds them in)"""
        return (f"---------------- {i} ----------------\n      Loss: {float(np.float32(loss)):g}\n"
                f"      Error: {float(np.float32(error)):g}\n-------------------------------------\n\n")

    def close(self) -> None:
        if self._h:
            lib().rt_dqn_fit_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def td_targets_device(ctx: Context, seed: int, next_q_ptr: int, terminal_ptr: int, reward_ptr: int,
                      discount_ptr: int, pix_ptr: int, sample: int, bounce: int, n: int, target_ptr: int,
                      stream: int = 0) -> None:
    """compute_td_targets (rt_dqn_td_targets_device) on device buffers."""
    v = ctypes.c_void_p
    check(lib().rt_dqn_td_targets_device(ctx.handle, seed, v(next_q_ptr), v(terminal_ptr), v(reward_ptr),
                                         v(discount_ptr), v(pix_ptr), sample, bounce, n, v(target_ptr),
                                         v(stream)))
