"""The DQN forward (k_dqn_mlp, k_dqn_mlp_ws) bit for bit, on networks where it is exact.

The restatement oracle.dqn_forward(bf16=True) accumulates each layer in fp64; the device
accumulates in fp32 on the MFMA in an order of its own.  On two families of networks fp32
accumulation is exact in every order, so the two must agree to the bit:

  * integer networks (rtmi.dqn.exact_weights): integer weights and biases, vertices and ray
    positions on the grid of eighths.  Every product and partial sum is a multiple of
    g = 1/8, bf16 rounding keeps it one, and while sum_i |w_i a_i| + |b| <= 2^24 g every
    partial sum is an fp32 number.  The CPU tests assert that bound with a margin of 4 on
    every network and batch the GPU tests use, that the networks are not trivial, that a
    plain numpy restatement with fp32 sums in three orders equals the oracle, and that the
    comparison sees seeded indexing faults.
  * selection networks (rtmi.dqn.selection_weights): a real layer 0 (the trained door room
    model, He-normal weights on the archway) on real surface points, with 0/1 selection
    matrices behind it: Q[a] = h1[sel[a]], the folded layer 0 (mlp_layer0, the fp32 MFMA)
    against the restatement's fmaf chain.

The hidden widths reach both bodies of k_dqn_mlp (the unrolled ring of the reference's padded
224-320-224 and the generic K loop) at every K-step count and N-tile slot pattern; the ray
counts sit around the 16-row M-tile, the weight-stationary kernel's 32-row tile and the
streaming kernel's workgroup (rt_dqn_mlp_rows).
"""
import functools
import os

import numpy as np
import pytest

from conftest import MODELS
from test_dqn import room_points, trained

F32, F64 = np.float32, np.float64

#           hidden            what it reaches
TRIPLES = [
    (200, 300, 200),  # the reference: unrolled body, zero padding in K
    (224, 320, 224),  # same body, no padding: the pad columns carry data
    (193, 289, 193),  # same body, the smallest widths that still pad to it
    (200, 300, 192),  # generic body near the maximal widths, all five N-tile slots in use
    (32, 32, 32),     # generic body, one K step: tail only
    (64, 64, 64),     # two K steps: loop without tail
    (96, 160, 96),    # odd step counts: loop plus tail
    (33, 31, 65),     # ragged widths
    (1, 1, 1),        # lone features
    (7, 9, 6),        # test_dqn._tiny_net's
]
N_INS = (12, 918)
FILLS = ("dense", "sparse")
NETS = [(h, n_in, fill) for h in TRIPLES for n_in in N_INS for fill in FILLS]
BASE_COUNTS = (1, 15, 16, 17, 31, 32, 33, 95, 96, 97, 191, 193, 1000)
BIG_COUNT = 49_153  # reference-shape triples: more workgroups than one resident wave of them
GRID = 0.125
LIMIT = 2.0 ** 24 * GRID  # sum |w a| + |b| up to which every fp32 partial sum is exact
MARGIN = 4.0


def net_id(p):
    return "-".join(str(x) for x in p[0]) + f"-in{p[1]}-{p[2]}"


def is_ref(hidden):
    return tuple((h + 31) // 32 * 32 for h in hidden) == (224, 320, 224)


assert [is_ref(h) for h in TRIPLES] == [True] * 3 + [False] * 7  # the bodies the table names


def max_count(hidden):
    return BIG_COUNT if is_ref(hidden) else max(BASE_COUNTS)


def ray_counts(hidden, rows):
    """the listed counts, both sides of the build's workgroup size and of two workgroups"""
    c = set(BASE_COUNTS) | {rows - 1, rows, rows + 1, 2 * rows - 1, 2 * rows + 1}
    if is_ref(hidden):
        c.add(BIG_COUNT)
    return sorted(x for x in c if x > 0)


# A random integer network can leave the feature a fault touches dead on every ray (a lone
# feature, the one real column of a layer's last K step): these networks take the first
# seed, in steps of 100, with which the two CPU tests below pass.
SEED_STEPS = {((200, 300, 200), 918, "sparse"): 1, ((33, 31, 65), 12, "sparse"): 1,
              ((1, 1, 1), 918, "dense"): 1, ((7, 9, 6), 918, "dense"): 1}


@functools.lru_cache(maxsize=None)
def network(hidden, n_in, fill):
    import rtmi
    seed = 1984 + 4 * TRIPLES.index(hidden) + (n_in == 918) + 2 * (fill == "sparse")
    seed += 100 * SEED_STEPS.get((hidden, n_in, fill), 0)
    return rtmi.dqn.exact_weights(n_in, hidden, fill, seed=seed)


@functools.lru_cache(maxsize=2)
def rays(n):
    import rtmi
    return rtmi.dqn.grid_points(n)


# ---- the plain numpy restatement ------------------------------------------------

def bf16_round(x):
    """round to nearest even to bf16 (finite values), as the oracle's bf16_round"""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(F32)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product is exact in fp64, TwoSum gives the fp64
    sum's error, and rounding the sum to odd before the cast to fp32 makes the two roundings
    one (53 >= 24 + 2 bits)"""
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    bits = bits + np.where(fix, np.where((e > 0) == (s > 0), 1, -1), 0)
    return bits.view(F64).astype(F32)


def fold_layer0(W0, b0, verts):
    """rt_dqn_create's fold: c0 = b + sum w v and S[c] = sum of w over coordinate c, in fp64
    in index order, rounded to fp32"""
    w, v = W0.astype(F64), np.asarray(verts, F64)
    c0 = np.cumsum(np.concatenate([np.asarray(b0, F64)[:, None], w * v[None, :]], axis=1), axis=1)[:, -1]
    S = [np.cumsum(w[:, c::3], axis=1)[:, -1].astype(F32) for c in range(3)]
    return c0.astype(F32), S


def ksum(prod, order):
    """sum of prod (.., K) over K in fp32: index order, reversed, or 32-wide chunks whose
    sums are then added in order"""
    if order == "reversed":
        prod = prod[..., ::-1]
    if order == "chunks":
        K = prod.shape[-1]
        pad = np.zeros(prod.shape[:-1] + ((-K) % 32,), F32)
        prod = np.concatenate([prod, pad], axis=-1).reshape(prod.shape[:-1] + (-1, 32))
        prod = np.cumsum(prod, axis=-1, dtype=F32)[..., -1]
    return np.cumsum(prod, axis=-1, dtype=F32)[..., -1]


FAULTS = ("swap_k", "drop_last_k", "swap_n_tiles", "zero_bias_tile", "swap_m_rows", "negate_w3")


def fault_applies(kind, layer, dims, n):
    """whether the network has what the fault exchanges: two K columns, two N tiles, a
    second M-tile of rays"""
    K, N = dims[layer], dims[layer + 1]
    return {"swap_k": K >= 2, "drop_last_k": True, "swap_n_tiles": N > 16, "zero_bias_tile": True,
            "swap_m_rows": layer == 3 and n > 19, "negate_w3": layer == 3}[kind]


def np_layer0(W0, b0, verts, loc, stats=None):
    """h1 = bf16(ReLU(cf - fmaf(s2, z, fmaf(s1, y, s0 * x)))) of the folded layer 0"""
    cf, S = fold_layer0(W0, b0, verts)
    x, y, z = loc[:, 0:1], loc[:, 1:2], loc[:, 2:3]
    pre = cf[None, :] - fma32(S[2][None, :], z, fma32(S[1][None, :], y, S[0][None, :] * x))
    act = np.maximum(pre, F32(0))
    if stats is not None:
        fold = np.abs(W0.astype(F64)) @ np.abs(np.asarray(verts, F64)) + np.abs(b0.astype(F64))
        reach = sum(np.abs(S[c].astype(F64))[None, :] * np.abs(loc[:, c:c + 1].astype(F64)) for c in range(3))
        stats.append((float((fold[None, :] + reach).max()), float((pre > 0).mean()),
                      int((act != bf16_round(act)).sum())))
    return bf16_round(act)


def np_forward(W, b, verts, loc, order="f64", fault=None, stats=None):
    """The bf16 forward in numpy: the host fold and the fmaf chain of layer 0, bf16 weights
    and activations, each layer's K summed in fp32 in `order` (ksum), or as one fp64 matrix
    product (exact on these networks; the fast path of the fault and condition tests).
    fault = (kind, layer) applies one indexing fault; stats collects, per layer, the bound
    max(sum |w a| + |b|), the fraction of positive pre-activations and the number of
    activations that bf16 rounding altered (an upper estimate of the bound, from an fp32
    product of the absolute values)."""
    loc = np.ascontiguousarray(loc, F32).reshape(-1, 3)
    a = np_layer0(W[0], b[0], verts, loc, stats)
    for l in range(1, 4):
        Wb, bias = bf16_round(W[l]), np.array(b[l], F32)
        kind = fault[0] if fault is not None and fault[1] == l else None
        K, N = Wb.shape[1], Wb.shape[0]
        if kind == "swap_k":     # two K columns read in each other's place
            Wb = Wb.copy()
            Wb[:, [0, K - 1]] = Wb[:, [K - 1, 0]]
        if kind == "drop_last_k":  # the last 32-wide K step never accumulated
            Wb = Wb.copy()
            Wb[:, (K - 1) // 32 * 32:] = 0
        if kind == "zero_bias_tile":
            bias[(N - 1) // 16 * 16:] = 0
        if kind == "negate_w3":
            Wb = Wb.copy()
            r, c = np.argwhere(Wb != 0)[len(np.argwhere(Wb != 0)) // 2]
            Wb[r, c] = -Wb[r, c]
        if order == "f64":
            acc = (a.astype(F64) @ Wb.astype(F64).T).astype(F32)
        elif order == "f32":  # an fp32 matrix product in the library's own order
            acc = a @ Wb.T
        else:
            acc = ksum(a[:, None, :] * Wb[None, :, :], order)
        pre = acc + bias[None, :]
        act = np.maximum(pre, F32(0))
        if stats is not None:
            # (non-negative terms: the fp32 product's relative error is below K 2^-24 < 1e-4)
            bound = (np.abs(a) @ np.abs(Wb).T).max() * (1 + 1e-4) + np.abs(bias).max()
            stats.append((float(bound), float((pre > 0).mean()), int((act != bf16_round(act)).sum())))
        a = bf16_round(act) if l < 3 else act
        if kind == "swap_n_tiles":  # the rows of two 16-row N tiles stored in each other's place
            w = min(16, N - 16)
            a = a.copy()
            a[:, :w], a[:, 16:16 + w] = a[:, 16:16 + w].copy(), a[:, :w].copy()
        if kind == "swap_m_rows":   # two rays' outputs exchanged across a 16-row M tile
            a = a.copy()
            a[[3, 19]] = a[[19, 3]]
    return a


def bits(q):
    return np.ascontiguousarray(q, F32).view(np.uint32)


# ---------------------------------------------------------------- CPU ----------

@pytest.mark.parametrize("net", NETS, ids=net_id)
def test_exactness_condition_and_nontrivial(rtmi_mod, net):
    """sum |w a| + |b| <= 2^24 g / 4 at every layer, ray and output of every network and batch
    the GPU tests use (g = 1/8: the limit is 2^21, the margin leaves 2^19); and the networks
    are worth comparing: a tenth of the pre-activations of every layer positive at least
    (about half of them, 0.3 to 0.7, in networks of 32 features a layer and more), bf16
    rounding at work in layers 1 and 2 of those, every ray with some Q > 0, and the rays
    distinct grid points."""
    hidden, n_in, fill = net
    W, b, verts = network(*net)
    n = max_count(hidden)
    assert max(ray_counts(hidden, rtmi_mod.dqn.mlp_rows())) == n
    loc = rays(n)
    cell = np.round(loc / GRID).astype(np.int64) + 32
    assert len(np.unique((cell[:, 0] * 65 + cell[:, 1]) * 65 + cell[:, 2])) == n
    for arr in (verts, loc):
        assert np.array_equal(arr / GRID, np.round(arr / GRID)) and np.abs(arr).max() <= 4.0
    for arr in W + b:
        assert np.array_equal(arr, np.round(arr))
    assert [w.shape for w in W] == list(zip((*hidden, 144), (n_in, *hidden)))
    if fill == "dense":
        assert all(np.count_nonzero(w) == w.size for w in W[1:])
    stats = []
    # (fp32 products: exact in any order once the bound of the same layer holds)
    q = np_forward(W, b, verts, loc, order="f32", stats=stats)
    print(net_id(net), "bounds", [s[0] for s in stats], "limit", LIMIT, "positive", [round(s[1], 3) for s in stats],
          "rounded", [s[2] for s in stats])
    for l, (bound, positive, rounded) in enumerate(stats):
        assert bound * MARGIN <= LIMIT, (l, bound)
        assert positive >= 0.1, (l, positive)  # (a lone feature with a positive bias may always be on)
        if min(hidden) >= 32:
            assert 0.3 <= positive <= 0.7, (l, positive)
            assert l not in (1, 2) or rounded > 0, l
    assert np.all(q.max(axis=1) > 0)


@pytest.mark.parametrize("net", NETS, ids=net_id)
def test_restatement_equals_oracle_in_any_order(oracle_mod, net):
    """The numpy restatement with each layer's K summed in fp32 in index order, reversed and
    in 32-wide chunks, and as an fp64 product, equals oracle.dqn_forward(bf16=True) bit for
    bit: on these networks the order of an fp32 accumulation cannot matter."""
    W, b, verts = network(*net)
    loc = rays(max_count(net[0]))[:33]
    want = bits(oracle_mod.dqn_forward(W, b, verts, loc, bf16=True))
    for order in ("forward", "reversed", "chunks", "f64"):
        assert np.array_equal(bits(np_forward(W, b, verts, loc, order=order)), want), order


@pytest.mark.parametrize("net", NETS, ids=net_id)
def test_seeded_faults_are_seen(net):
    """Each indexing fault, applied in the numpy restatement at each layer that has what it
    exchanges, changes at least one bit of Q on the batch the GPU test compares."""
    hidden, n_in, fill = net
    W, b, verts = network(*net)
    loc = rays(max_count(hidden))[:max(BASE_COUNTS)]
    dims = (n_in, *hidden, 144)
    good = bits(np_forward(W, b, verts, loc))
    tried = set()
    for kind in FAULTS:
        for layer in (1, 2, 3):
            if not fault_applies(kind, layer, dims, len(loc)):
                continue
            tried.add(kind)
            bad = bits(np_forward(W, b, verts, loc, fault=(kind, layer)))
            assert not np.array_equal(bad, good), (kind, layer)
    assert tried >= {"drop_last_k", "zero_bias_tile", "swap_m_rows", "negate_w3"}
    assert min(hidden) < 32 or tried == set(FAULTS)


# ---- selection networks: layer 0 on real data ----

SELECTIONS = (0, 56)  # features 0-143 and 56-199: all 200
SEL_HIDDEN = ((200, 300, 200), (200, 144, 144))  # the reference-shape body, the generic one
SEL_NETS = [(k, s, h) for k in ("door_room", "archway") for s in SELECTIONS for h in SEL_HIDDEN]


@functools.lru_cache(maxsize=None)
def scene_layer0(kind):
    import rtmi
    g = rtmi.obj_geometry(os.path.join(MODELS, f"{kind}.obj"), kind)
    W, b = trained(rtmi) if kind == "door_room" else rtmi.dqn.synthetic_weights(g.nn_vertices.size)
    return g, W[0], b[0]


def selection_net(kind, first, hidden):
    import rtmi
    g, W0, b0 = scene_layer0(kind)
    W, b = rtmi.dqn.selection_weights(W0, b0, np.arange(first, first + 144), hidden)
    return g, W, b


def sel_id(p):
    return f"{p[0]}-from{p[1]}-" + "-".join(str(x) for x in p[2])


@pytest.mark.parametrize("net", SEL_NETS, ids=sel_id)
def test_selection_networks_select_layer0(oracle_mod, net):
    """Q[a] = h1[first + a] of the restatement, bit for bit, in numpy and in the oracle, with
    h1 the bf16-rounded ReLU of the folded layer 0's fmaf chain on real surface points (no
    exactness condition to meet: every sum of layers 1-3 has one term); layer 0 is alive."""
    kind, first, hidden = net
    g, W, b = selection_net(*net)
    pts, _ = room_points(g, 777, 3)
    q = oracle_mod.dqn_forward(W, b, g.nn_vertices, pts, bf16=True)
    assert np.array_equal(bits(np_forward(W, b, g.nn_vertices, pts)), bits(q))
    h1 = np_layer0(W[0], b[0], g.nn_vertices, pts)
    assert np.array_equal(bits(q), bits(h1[:, first:first + 144]))
    assert 0.05 < (q > 0).mean() < 0.95 and len(np.unique(bits(q))) > 1000
    assert not np.array_equal(q, np.round(q / GRID) * GRID)  # ordinary floats, not grid values


# ---------------------------------------------------------------- GPU ----------

@pytest.mark.gpu
@pytest.mark.parametrize("net", NETS, ids=net_id)
def test_gpu_forward_bit_exact_integer_networks(rtmi_mod, oracle_mod, gpu_ctx, net):
    """net.forward equals the restatement bit for bit at every ray count, on the streaming
    kernel and, for the reference's padded shape, on the weight-stationary one; on a generic
    shape asking for the stationary kernel changes nothing (it does not fit, so the streaming
    kernel runs).  One Dqn and one reference per network, the batches its prefixes."""
    hidden, n_in, fill = net
    W, b, verts = network(*net)
    counts = ray_counts(hidden, rtmi_mod.dqn.mlp_rows())
    loc = rays(max(counts))
    want = bits(oracle_mod.dqn_forward(W, b, verts, loc, bf16=True))
    with rtmi_mod.dqn.Dqn(gpu_ctx, verts, W, b) as dq:
        for mode in (dq.MLP_STREAM, dq.MLP_STATIONARY):
            dq.set_mlp(mode)
            for n in counts:
                got = bits(dq.forward(loc[:n]))
                bad = np.argwhere(got != want[:n])
                assert bad.size == 0, (mode, n, len(bad), bad[:8].tolist(),
                                       got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.gpu
@pytest.mark.parametrize("net", SEL_NETS, ids=sel_id)
def test_gpu_layer0_bit_exact_on_selection_networks(rtmi_mod, oracle_mod, gpu_ctx, net):
    """The folded layer 0 (mlp_layer0: one v_mfma_f32_16x16x4_f32 per tile) against the
    restatement's cf - fmaf(s2, z, fmaf(s1, y, s0 * x)) on real surface points, read out
    through selection layers, on both kernels."""
    g, W, b = selection_net(*net)
    with rtmi_mod.dqn.Dqn(gpu_ctx, g.nn_vertices, W, b) as dq:
        for n in (777, 96):
            pts, _ = room_points(g, n, 3)
            want = bits(oracle_mod.dqn_forward(W, b, g.nn_vertices, pts, bf16=True))
            for mode in (dq.MLP_STREAM, dq.MLP_STATIONARY):
                dq.set_mlp(mode)
                got = bits(dq.forward(pts))
                bad = np.argwhere(got != want)
                assert bad.size == 0, (mode, n, len(bad), bad[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [(200, 300, 200), (96, 160, 96)], ids=["reference", "generic"])
def test_gpu_forward_device_leaves_guard_rows(rtmi_mod, oracle_mod, gpu_ctx, hidden):
    """rt_dqn_forward_device writes the n x 144 block and nothing else: guard rows of a
    sentinel pattern before and after it stay untouched (padding rows of the last workgroup
    may be written only in the renderer's action-major layout, which this entry point does
    not use), on both kernels."""
    torch = pytest.importorskip("torch")
    W, b, verts = network(hidden, 12, "dense")
    sentinel, guard = 0x7FC5A5A5, 256
    with rtmi_mod.dqn.Dqn(gpu_ctx, verts, W, b) as dq:
        for n in (1, 97, 193):
            loc = rays(max_count(hidden))[:n]
            want = bits(oracle_mod.dqn_forward(W, b, verts, loc, bf16=True))
            d_loc = torch.from_numpy(loc).cuda()
            for mode in (dq.MLP_STREAM, dq.MLP_STATIONARY):
                dq.set_mlp(mode)
                buf = torch.full((guard + n + guard, 144), sentinel, dtype=torch.int32, device="cuda")
                dq.forward_device(d_loc.data_ptr(), n, buf[guard].data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                out = buf.cpu().numpy().view(np.uint32)
                assert np.array_equal(out[guard:guard + n], want), (mode, n)
                assert np.all(out[:guard] == sentinel) and np.all(out[guard + n:] == sentinel), (mode, n)
