"""The Neural-Q trainer (csrc/rt_train.hip) element by element: the gradients of one step
against the fp64 restatement (oracle.AdamRef.loss_grads) and the Adam update against an fp64
recomputation from the device's own gradients, at the shapes where the kernels take another
path: split-K of 1, 2, 10, 16 and 64 slices (k_sum_slices' 8-wide loop and its remainder),
lengths that are no multiple of 4 (its scalar tail), widths below and just off the 64 tile,
batches of 1, 3, 63..65 rays, the K / 256 thresholds of split_for, a ragged last slice,
row chunks above 64 rows, both branches of the clip, the all-ignored batch, workspace growth
and reuse.

Inputs.  A fp32 ReLU network and its fp64 reference may legitimately disagree when a
pre-activation sits on zero (one flipped unit moves a gradient block by 1e-3 and more), so
every batch is built clear of that edge: 1.5 n + 64 candidate rays uniform in [-1, 1]^3, the
first n whose smallest |pre-activation| over the four layers (fp64) is >= 1e-4 are the batch
(a fp32 pre-activation is off by ~1e-6).  All n rays go to the device and all are compared.
act[::97] = -1 and act[1] = n_out + 3 are ignored rows (n >= 3), the last ray is live (its
action is its largest Q), and with n >= 64 at least 3 picked outputs are dead (q_a = 0: they
count in the loss and give no gradient).  Networks: A 12-7-9-6-10 and B 30-65-130-63-144,
He-normal weights, biases 0.1, vertices uniform in [-1, 1]; C is door_room.obj's nn_vertices
with synthetic_weights(342) (342-200-300-200-144).

Gradient criterion.  grad_error() is the worst, over the 8 blocks dW0..dW3, db0..db3, of
max|g - g_ref| / max|g_ref|, and the loss' relative error; a block that is exactly zero in
the reference must be exactly zero.  tol(case) = TOL below.  Each entry is 16 x the larger of
the two errors of the pure-numpy fp32 restatement (oracle.loss_grads_f32: numpy's own sums;
strict per-ray chains cut into the device's split-K slices) against fp64 on that case's
batch, rounded up to two digits; measured on the CPU (units of 1e-7):

    case             numpy  chain  TOL       case             numpy  chain  TOL
    A-1               3.13   3.13  5.1e-6    B-511             5.00   4.92  8.0e-6
    A-3               4.05   4.05  6.5e-6    B-512             7.49   7.49  1.2e-5
    A-64              2.89   3.31  5.3e-6    B-513             5.67   5.67  9.1e-6
    A-513             2.50   1.74  4.0e-6    B-16641          21.65  21.65  3.5e-5
    B-63              2.81   2.81  4.6e-6    C-2561           16.96  16.96  2.8e-5
    B-64              4.70   4.73  7.6e-6    C-4096            9.51   9.51  1.6e-5
    B-65              4.30   4.30  6.9e-6    A-3-unclipped     7.19   7.19  1.2e-5
    B-255             4.43   5.69  9.2e-6    A-64-unclipped   42.77  42.77  6.9e-5
    B-256             5.22   5.75  9.2e-6    A-513-unclipped  40.97  43.41  7.0e-5
    B-257             4.72   4.72  7.6e-6

(where the two orders agree, a block or the loss that does not depend on the order of the
weight-gradient sums is the worst.  The unclipped batches' targets lie within ~0.03 of the
network's own outputs, so the fp32 rounding of q_a is a larger part of target - q_a; they use
net A, whose few parameters leave the largest delta at ||g|| = 2: on net B the same rule
gives 16 x 5e-5, no longer a tenth of the smallest seeded error).  Why 16: the device's layer 1-3 forward
and dH products are k-ordered fma chains of up to 300 terms where numpy sums in blocks, and
fma rounds differently from mul + add.  The seeded errors of
test_criterion_rejects_seeded_errors (rolled edge rows, a zeroed tail, a lost slice, y/z
exchanged in layer 0, a dropped last ray) land between 5.7e-3 and 0.56, two orders and more
above every entry; test_tolerances_are_16x_fp32_error recomputes both sides.  The numbers
are not tuned against the device.

Adam criterion (teacher-forced).  After every step the host recomputes m, v, the clip scale
5 / ||g|| (||g|| as the device reported it), lr_t and the update in fp64 from the gradients
the device read out, with the hyper-parameters as the ABI holds them (floats), and carries
its own parameters from the initial ones.  Every parameter must agree within
T (1e-5 lr + ulp32(|x|)) after T steps: per step the update, of magnitude <= ~lr, goes through
at most ~90 fp32 roundings of relative size 2^-24 (the two moment recurrences with their
scale products, sqrt, + eps, divide, times lr_t, and the rounding carried in m and v from
earlier steps, which decays with beta1, beta2) -- 90 x 6e-8 = 5.4e-6 < 1e-5 -- plus one
rounding of x.  A bias correction that is one step ahead moves the first update by 0.26 lr
(lr_2 m / sqrt(v) with zero moments before is 0.744 lr where lr_1 gives lr), four orders
above the tolerance (test_host_adam_is_the_restatement_and_sees_an_off_by_one); beta2 taken as 0.999 in double
instead of the float the device holds moves sqrt(v) by 5e-6.
"""
import functools
import os

import numpy as np
import pytest

from conftest import MODELS

LR = float(np.float32(1e-3))
MARGIN = 1e-4
NETS = {"A": (12, 7, 9, 6, 10), "B": (30, 65, 130, 63, 144)}
CASES = [("A", 1), ("A", 3), ("A", 64), ("A", 513),
         ("B", 63), ("B", 64), ("B", 65), ("B", 255), ("B", 256), ("B", 257), ("B", 511), ("B", 512),
         ("B", 513), ("B", 16641), ("C", 2561), ("C", 4096)]
# 16 x the fp32 restatement's error (module docstring), never the device's
TOL = {
    "A-1": 5.1e-6, "A-3": 6.5e-6, "A-64": 5.3e-6, "A-513": 4.0e-6,
    "B-63": 4.6e-6, "B-64": 7.6e-6, "B-65": 6.9e-6, "B-255": 9.2e-6, "B-256": 9.2e-6, "B-257": 7.6e-6,
    "B-511": 8.0e-6, "B-512": 1.2e-5, "B-513": 9.1e-6, "B-16641": 3.5e-5, "C-2561": 2.8e-5, "C-4096": 1.6e-5,
    "A-3-unclipped": 1.2e-5, "A-64-unclipped": 6.9e-5, "A-513-unclipped": 7.0e-5,
}
SEEDED = [("A", 513), ("B", 257), ("C", 2561)]  # one n per net for the seeded errors
SEEDS = {("A", 1): 0}  # a single ray that is live in the reference


def _id(case):
    return "-".join(str(x) for x in case)


@functools.lru_cache(maxsize=None)
def _net(name):
    """(nn_vertices, [W0..W3], [b0..b3]) in float32"""
    if name == "C":
        import rtmi
        g = rtmi.obj_geometry(os.path.join(MODELS, "door_room.obj"), "door_room")
        W, b = rtmi.dqn.synthetic_weights(g.nn_vertices.size)
        assert g.nn_vertices.size == 342
        return np.ascontiguousarray(g.nn_vertices, np.float32).ravel(), W, b
    dims = NETS[name]
    rng = np.random.default_rng({"A": 101, "B": 102}[name])
    W = [(rng.standard_normal((dims[i + 1], dims[i])) * np.sqrt(2.0 / dims[i])).astype(np.float32)
         for i in range(4)]
    b = [np.full(dims[i + 1], 0.1, np.float32) for i in range(4)]
    return rng.uniform(-1, 1, dims[0]).astype(np.float32), W, b


def _ref(name):
    import oracle
    return oracle.AdamRef(*_net(name), lr=LR)


@functools.lru_cache(maxsize=None)
def _batch(name, n, seed=None, unclipped=False):
    """A batch built by the module docstring's rule with its fp64 loss and gradients:
    dict(loc, act, tgt, loss, G, gn).  Cached: the reference is computed once and shared."""
    ref = _ref(name)
    if seed is None:
        seed = SEEDS.get((name, n), 1000 + n)
    rng = np.random.default_rng(seed)
    n_out = ref.P[3].shape[0]
    cand = rng.uniform(-1, 1, (int(1.5 * n) + 64, 3)).astype(np.float32)
    margin = np.min([np.abs(z).min(axis=1) for z in ref.preactivations(cand)], axis=0)
    keep = np.nonzero(margin >= MARGIN)[0]
    assert keep.size >= n, (keep.size, n)
    loc = np.ascontiguousarray(cand[keep[:n]])
    q = ref.forward(loc)[4]
    act = rng.integers(0, n_out, n).astype(np.int32)
    if n >= 3:
        assert (n - 1) % 97 != 0
        act[::97] = -1
        act[1] = n_out + 3
    act[-1] = int(np.argmax(q[-1]))
    ok = (act >= 0) & (act < n_out)
    qa = np.where(ok, q[np.arange(n), np.where(ok, act, 0)], 0.0)
    if unclipped:  # targets = q_a + delta, delta scaled so that ||g|| is about 2
        delta = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
        _, G = ref.loss_grads(loc, act, qa + delta)
        delta *= 2.0 / np.sqrt(sum(float(np.sum(g * g)) for g in G))
        tgt = (qa + delta).astype(np.float32)
    else:
        tgt = rng.uniform(0.0, 2.0, n).astype(np.float32)
    loss, G = ref.loss_grads(loc, act, tgt)
    gn = float(np.sqrt(sum(float(np.sum(g * g)) for g in G)))
    # the conditions on the reference, before any device sees the batch
    assert q[-1, act[-1]] > 0.0 and tgt[-1] != q[-1, act[-1]], "the last ray must have a gradient row"
    if n >= 64:
        assert np.count_nonzero(ok & (qa == 0.0)) >= 3, "at least 3 dead picked outputs"
    if n >= 3:
        assert act[0] == -1 and act[1] >= n_out
    for a in (loc, act, tgt):
        a.setflags(write=False)
    return dict(name=name, n=n, loc=loc, act=act, tgt=tgt, loss=loss, G=G, gn=gn)


def grad_error(G, loss, G_ref, loss_ref):
    """The gradient criterion: the worst of max|g - g_ref| / max|g_ref| over the 8 blocks and
    of the loss' relative error; inf where a block that is exactly zero in the reference is
    not, or where a value is not finite."""
    if not np.isfinite(loss):
        return float("inf")
    if loss_ref == 0.0:
        worst = 0.0 if loss == 0.0 else float("inf")
    else:
        worst = abs(float(loss) - loss_ref) / abs(loss_ref)
    assert len(G) == len(G_ref) == 8
    for g, r in zip(G, G_ref):
        g = np.asarray(g, np.float64)
        assert g.shape == r.shape, (g.shape, r.shape)
        if not np.all(np.isfinite(g)):
            return float("inf")
        den = float(np.abs(r).max())
        if den == 0.0:
            e = 0.0 if not g.any() else float("inf")
        else:
            e = float(np.abs(g - r).max()) / den
        worst = max(worst, e)
    return worst


def _seeded_errors(bt):
    """name -> (loss, gradients): the reference's own gradients with one error each"""
    G, n = bt["G"], bt["n"]
    out = {}
    c = [g.copy() for g in G]
    c[1][-3:] = np.roll(c[1][-3:], 1, axis=0)
    out["last 3 rows of dW1 rolled"] = (bt["loss"], c)
    c = [g.copy() for g in G]
    c[5][-2:] = 0.0
    out["last 2 entries of db1 zeroed"] = (bt["loss"], c)
    c = [g.copy() for g in G]
    c[3] *= 1.0 - 1.0 / 64.0
    out["one of 64 slices of dW3 lost"] = (bt["loss"], c)
    # dW0[o][j] = db0[o] v_j - T[o][j % 3]: T from columns 0..2, y and z exchanged
    v = _net(bt["name"])[0].astype(np.float64)
    T = G[4][:, None] * v[None, :3] - G[0][:, :3]
    c = [g.copy() for g in G]
    c[0] = G[4][:, None] * v[None, :] - np.tile(T[:, [0, 2, 1]], (1, v.size // 3))
    assert np.allclose(G[4][:, None] * v[None, :] - np.tile(T, (1, v.size // 3)), G[0], rtol=0, atol=1e-9 * np.abs(G[0]).max())
    out["y and z exchanged in layer 0"] = (bt["loss"], c)
    out["last ray dropped"] = _ref(bt["name"]).loss_grads(bt["loc"][:n - 1], bt["act"][:n - 1], bt["tgt"][:n - 1])
    return out


@functools.lru_cache(maxsize=None)
def _fp32_errors(name, n, unclipped=False):
    """(numpy order, chain order): grad_error of the fp32 restatement against fp64"""
    import oracle
    bt = _batch(name, n, unclipped=unclipped)
    v, W, b = _net(name)
    return tuple(grad_error(G, float(loss), bt["G"], bt["loss"])
                 for loss, G in (oracle.loss_grads_f32(v, W, b, bt["loc"], bt["act"], bt["tgt"], order=o)
                                 for o in ("numpy", "chain")))


UNCLIPPED = [("A", 3, True), ("A", 64, True), ("A", 513, True)]
TOL_CASES = [(nm, n, False) for nm, n in CASES] + UNCLIPPED


def _tol_id(c):
    return _id(c[:2]) + ("-unclipped" if c[2] else "")


# --- CPU: the criterion and its tolerances --------------------------------------

def test_batches_keep_the_margin_and_the_table_is_complete(oracle_mod):
    assert sorted(TOL) == sorted(_tol_id(c) for c in TOL_CASES)
    for name, n, unc in TOL_CASES:
        bt = _batch(name, n, unclipped=unc)
        zs = _ref(name).preactivations(bt["loc"])
        assert bt["loc"].shape == (n, 3) and min(float(np.abs(z).min()) for z in zs) >= MARGIN
        if unc:
            assert 0.05 <= bt["gn"] <= 2.5, bt["gn"]
        elif n >= 63:
            assert bt["gn"] > 10.0, bt["gn"]


def test_split_for_restated(oracle_mod):
    """the slice counts the shapes are chosen for (rt_train.hip split_for restated)"""
    s = oracle_mod.train_split_for
    assert [s(130, 65, n) for n in (511, 512, 513, 2561, 16641)] == [1, 2, 2, 10, 64]
    assert s(10, 6, 513) == 2 and s(10, 6, 511) == 1
    assert s(300, 200, 2561) == 10 and s(300, 200, 4096) == 16 and s(200, 300, 65536) == 52
    assert s(144, 200, 777) == 3 and s(7, 12, 1) == 1


@pytest.mark.parametrize("case", SEEDED, ids=_id)
def test_criterion_rejects_seeded_errors(oracle_mod, case):
    """Block-level errors seeded into the reference's own gradients are rejected at the
    case's tolerance, and the fp32 restatement in both summation orders is accepted."""
    bt = _batch(*case)
    tol = TOL[_id(case)]
    assert grad_error(bt["G"], bt["loss"], bt["G"], bt["loss"]) == 0.0
    for what, (loss, G) in _seeded_errors(bt).items():
        e = grad_error(G, loss, bt["G"], bt["loss"])
        print(f"{_id(case)} {what}: {e:.3g}")
        assert e > tol, (what, e, tol)
    for order, e in zip(("numpy", "chain"), _fp32_errors(*case)):
        print(f"{_id(case)} fp32 {order}: {e:.3g}")
        assert e <= tol, (order, e, tol)
    # a block that is zero in the reference must be zero: one ulp-sized value is refused
    Z = [np.zeros_like(g) for g in bt["G"]]
    Z2 = [z.copy() for z in Z]
    Z2[6][0] = 1e-30
    assert grad_error(Z, 0.0, Z, 0.0) == 0.0 and grad_error(Z2, 0.0, Z, 0.0) == float("inf")


@pytest.mark.parametrize("case", TOL_CASES, ids=_tol_id)
def test_tolerances_are_16x_fp32_error(oracle_mod, case):
    """TOL is what the docstring says: at least 16 x the fp32 restatement's error on the
    case's batch (recomputed here) and at most a tenth of the smallest seeded error."""
    tol = TOL[_tol_id(case)]
    errs = _fp32_errors(*case)
    print(f"{_tol_id(case)} fp32 numpy {errs[0]:.3g} chain {errs[1]:.3g} tol {tol:.3g}")
    assert tol >= 16.0 * max(errs), (errs, tol)
    seeded = min(grad_error(G, loss, _batch(*c)["G"], _batch(*c)["loss"])
                 for c in SEEDED for loss, G in _seeded_errors(_batch(*c)).values())
    assert tol <= seeded / 10.0, (tol, seeded)


class _HostAdam:
    """dynet::AdamTrainer's update in fp64 from given gradients (module docstring)."""
    b1, b2, eps, clip = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8)), 5.0

    def __init__(self, W, b, lr=LR):
        self.X = [np.asarray(p, np.float64).copy() for p in list(W) + list(b)]
        self.M = [np.zeros_like(x) for x in self.X]
        self.V = [np.zeros_like(x) for x in self.X]
        self.lr, self.t = lr, 0

    def update(self, G, gn):
        self.t += 1
        s = self.clip / gn if gn > self.clip else 1.0
        lr_t = self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for i, g in enumerate(G):
            g = np.asarray(g, np.float64)
            self.M[i] = self.M[i] * self.b1 + g * ((1.0 - self.b1) * s)
            self.V[i] = self.V[i] * self.b2 + (g * g) * ((1.0 - self.b2) * (s * s))
            self.X[i] = self.X[i] - self.M[i] / (np.sqrt(self.V[i]) + self.eps) * lr_t

    def worst(self, P, T):
        """largest |x_device - x_host| in units of T (1e-5 lr + ulp32(|x|))"""
        w = 0.0
        for x, p in zip(self.X, P):
            p = np.asarray(p, np.float64)
            assert p.shape == x.shape and np.all(np.isfinite(p))
            tol = T * (1e-5 * self.lr + np.spacing(np.abs(x).astype(np.float32)).astype(np.float64))
            w = max(w, float((np.abs(p - x) / tol).max()))
        return w


def test_host_adam_is_the_restatement_and_sees_an_off_by_one(oracle_mod):
    """_HostAdam fed AdamRef's gradients follows AdamRef.step (up to the float
    hyper-parameters); a bias correction one step late misses the tolerance ~50-fold."""
    v, W, b = _net("A")
    bt = _batch("A", 64)
    ref, host, late = _ref("A"), _HostAdam(W, b), _HostAdam(W, b)
    late.t = 1
    for T in (1, 2, 3):
        _, G = ref.loss_grads(bt["loc"], bt["act"], bt["tgt"])
        _, gn = ref.step(bt["loc"], bt["act"], bt["tgt"])
        host.update(G, gn)
        late.update(G, gn)
        assert host.worst(ref.P, T) <= 1.0
        if T == 1:
            assert late.worst(ref.P, 1) > 20.0


# --- GPU ---------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached batches are read-only)


def _step(tr, bt):
    loc, act, tgt = _dev(bt["loc"]), _dev(bt["act"]), _dev(bt["tgt"])
    return tr.step_device(loc.data_ptr(), act.data_ptr(), tgt.data_ptr(), bt["n"])


def _trainer(rtmi_mod, gpu_ctx, name):
    v, W, b = _net(name)
    return rtmi_mod.dqn.DqnTrainer(gpu_ctx, v, W, b, learning_rate=LR)


def _check_gradients(tr, bt, loss, gn, tol):
    """check 1: read-out gradients and loss against the reference; the reported norm against
    the fp64 norm of the read-out gradients (a fixed-order blocked sum of non-negative terms,
    <= ~22 roundings: 1.3e-6, halved by the square root)"""
    Wg, bg = tr.grads()
    G = Wg + bg
    e = grad_error(G, loss, bt["G"], bt["loss"])
    norm = float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in G)))
    print(f"{bt['name']}-{bt['n']}: grad_error {e:.3g} (tol {tol:.3g}), |g| {gn:.9g} vs read-out {norm:.9g}, "
          f"reference {bt['gn']:.9g}")
    assert e <= tol, (e, tol)
    assert abs(gn - norm) <= 1e-5 * norm, (gn, norm)
    return G


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gradients_element_by_element(rtmi_mod, oracle_mod, gpu_ctx, case):
    """One step of a fresh trainer: every gradient element, the loss and the norm."""
    bt = _batch(*case)
    with _trainer(rtmi_mod, gpu_ctx, case[0]) as tr:
        with pytest.raises(Exception):
            tr.grads()  # no step has run
        loss, gn = _step(tr, bt)
        _check_gradients(tr, bt, loss, gn, TOL[_id(case)])


@pytest.mark.gpu
def test_teacher_forced_adam_over_different_batches(rtmi_mod, oracle_mod, gpu_ctx):
    """12 steps of net B on 12 different batches of 64, 2561, 64, 513, 513.. rays (the
    workspace grows, then serves smaller batches): after every step each parameter equals the
    fp64 Adam recomputed from the device's own gradients (module docstring)."""
    v, W, b = _net("B")
    host = _HostAdam(W, b)
    sizes = [64, 2561, 64, 513] + [513] * 8
    with _trainer(rtmi_mod, gpu_ctx, "B") as tr:
        for i, n in enumerate(sizes):
            bt = _batch("B", n, seed=2000 + i)
            loss, gn = _step(tr, bt)
            Wg, bg = tr.grads()
            host.update(Wg + bg, gn)
            Wp, bp = tr.params()
            w = host.worst(Wp + bp, i + 1)
            print(f"step {i + 1} n {n}: loss {loss:.6g} |g| {gn:.6g} worst {w:.3g} of the tolerance")
            assert w <= 1.0, (i + 1, w)
            if i == 0:  # the first batch is the fresh network's: its gradients are the reference's
                assert grad_error(Wg + bg, loss, bt["G"], bt["loss"]) <= TOL["B-64"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("B", 257, False)] + UNCLIPPED, ids=_tol_id)
def test_both_clip_branches(rtmi_mod, oracle_mod, gpu_ctx, case):
    """Clipped (targets uniform in [0, 2], ||g|| > 10) and unclipped (targets = q_a + delta,
    ||g|| in [0.05, 2.5], so the scale is 1): the gradients of the first step and three
    teacher-forced Adam steps."""
    name, n, unc = case
    bt = _batch(name, n, unclipped=unc)
    assert (0.05 <= bt["gn"] <= 2.5) if unc else bt["gn"] > 10.0
    v, W, b = _net(name)
    host = _HostAdam(W, b)
    with _trainer(rtmi_mod, gpu_ctx, name) as tr:
        for T in (1, 2, 3):
            loss, gn = _step(tr, bt)
            if T == 1:
                G = _check_gradients(tr, bt, loss, gn, TOL[_tol_id(case)])
                assert (gn <= 5.0) if unc else (gn > 10.0)
            else:
                G = sum(tr.grads(), [])
            host.update(G, gn)
            Wp, bp = tr.params()
            w = host.worst(Wp + bp, T)
            print(f"step {T}: |g| {gn:.6g} worst {w:.3g} of the tolerance")
            assert w <= 1.0, (T, w)


@pytest.mark.gpu
def test_zero_gradient_step_then_a_normal_one(rtmi_mod, oracle_mod, gpu_ctx):
    """Every action ignored: loss 0, ||g|| 0, gradients exactly 0 and the parameters
    bit-identical (0 / (0 + eps) in the update).  The next, normal step matches the reference
    on the unchanged network and an Adam whose t the empty step advanced."""
    v, W, b = _net("B")
    bt = _batch("B", 257)
    empty = dict(bt, n=64, loc=bt["loc"][:64], act=np.full(64, -1, np.int32), tgt=bt["tgt"][:64])
    host = _HostAdam(W, b)
    with _trainer(rtmi_mod, gpu_ctx, "B") as tr:
        loss, gn = _step(tr, empty)
        assert loss == 0.0 and gn == 0.0
        G = sum(tr.grads(), [])
        assert all(not g.any() for g in G)
        P = sum(tr.params(), [])
        for p, p0 in zip(P, W + b):
            assert np.all(np.isfinite(p)) and np.array_equal(p.view(np.uint32), np.asarray(p0, np.float32).view(np.uint32))
        host.update(G, gn)
        loss, gn = _step(tr, bt)
        G = _check_gradients(tr, bt, loss, gn, TOL["B-257"])
        host.update(G, gn)
        assert host.t == 2
        w = host.worst(sum(tr.params(), []), 2)
        assert w <= 1.0, w
        skipped = _HostAdam(W, b)  # an Adam that did not count the empty step
        skipped.update(G, gn)
        assert skipped.worst(sum(tr.params(), []), 2) > 20.0


@pytest.mark.gpu
def test_step_is_deterministic_at_the_renderer_batch(rtmi_mod, oracle_mod, gpu_ctx):
    """Net C, 4096 rays (16 split-K slices), two fresh trainers: gradients and parameters
    bit-identical."""
    bt = _batch("C", 4096)
    runs = []
    for _ in range(2):
        with _trainer(rtmi_mod, gpu_ctx, "C") as tr:
            out = _step(tr, bt)
            runs.append((out, sum(tr.grads(), []) + sum(tr.params(), [])))
    assert runs[0][0] == runs[1][0]
    for a, c in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
