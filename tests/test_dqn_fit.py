"""The Q-network fit (csrc/rt_train.hip, rt_dqn_fit_*; the reference's NN_Q_Value_Trainer,
NN_Q_Value_Trainer/Source/main.cu:118-294): the split and shuffle, the Q-table reader, the dense
step element by element against an fp64 restatement, the held-out error, the epoch driver
against its own steps, and a fit of a small Cornell radiance map that goes on into the bf16
inference network.

Restatements.  dense_ref() is oracle.AdamRef's step with the dense loss in place of the picked
action: loss = sum_b sum_a (target - q)^2, output gradient q > 0 ? -2 (target - q) : 0, the
backward pass of AdamRef.loss_grads, in fp64 on AdamRef.forward.  dense_f32() is the same in
float32 with numpy alone (the input nn_vertices - loc built explicitly; order "numpy": every
contraction numpy's matmul, order "einsum": np.einsum's own loops, another summation order).
error_ref() / error_f32() are the test loop's sum_b ||target_b - Q(loc_b)||^2 (the fp32 one
squares and sums its fp32 differences in double, as the ABI states).

Inputs.  Networks A 12-7-9-6-10, B 30-65-130-63-144 and C (door_room, 342-200-300-200-144) and
the batch rule are tests/test_dqn_train.py's: 1.5 n + 64 candidate positions uniform in
[-1, 1]^3, the first n whose smallest |pre-activation| over the four layers (fp64) is >= 1e-4.
Targets are uniform in [0, 2] for every output, so with n >= 63 some outputs are dead (q = 0:
they count in the loss and pass no gradient) and most are live, and ||g|| > 10: the clip is
taken.  The "unclipped" batches' targets are the network's own outputs plus a delta scaled so
that ||g|| is about 2: the clip is not taken.

Gradient criterion and tolerances.  test_dqn_train.grad_error (the worst over the 8 blocks of
max|g - g_ref| / max|g_ref| and of the loss' relative error; an exactly zero block must be
exactly zero).  TOL[case] is 16 x the larger of the two orders' grad_error of dense_f32 against
dense_ref on that case's batch, rounded up to two digits -- test_dqn_train.py's rule, its
docstring has the reason for the 16 -- measured on the CPU (units of 1e-7):

    case             numpy einsum TOL       case             numpy einsum TOL
    A-1                3.28   4.67 7.5e-6   B-128              4.20   4.86 7.8e-6
    A-3                1.60   2.10 3.4e-6   B-129              5.14   3.34 8.3e-6
    A-64               3.72   3.52 6.0e-6   B-257              5.89   5.03 9.5e-6
    A-513              6.09   6.38 1.1e-5   B-513              5.24   6.29 1.1e-5
    B-1                5.15   6.71 1.1e-5   C-128              4.13   4.24 6.8e-6
    B-63               3.78   3.20 6.1e-6   A-3-unclipped     17.69  23.68 3.8e-5
    B-64               3.65   3.65 5.9e-6   A-64-unclipped   358.48 119.93 5.8e-4
    B-65               3.99   3.28 6.4e-6

(the unclipped batches use net A for test_dqn_train.py's reason, which the dense loss sharpens:
with every output in the loss, the delta that leaves ||g|| = 2 is a few 1e-3 at n = 64, so the
fp32 rounding of q is a large part of target - q; on net B at n = 65 the same rule gives 0.029,
above some of the seeded errors, and is not used.)

ERR_TOL[case] is the same rule for the held-out error: 16 x the larger relative error of
error_f32 (both orders) against error_ref (a sum of thousands of squares, whose rounding errors
average out: the entries lie below one fp32 ulp):

    case             numpy einsum ERR_TOL   case             numpy einsum ERR_TOL
    A-1                0.40   0.09 6.5e-7   A-4097             0.03   0.03 4.4e-8
    A-255              0.03   0.02 4.8e-8   B-1                0.17   0.74 1.2e-6
    A-256              0.04   0.02 6.1e-8   B-257              0.70   0.75 1.3e-6
    A-257              0.02   0.04 6.6e-8   B-4097             0.67   0.67 1.1e-6

test_tolerances_are_16x_fp32_error recomputes both tables.  No number here was measured
against the device.  The seeded errors of test_criterion_rejects_seeded_errors (no q > 0 mask,
a factor 1 for 2, the last row dropped, the targets' columns rolled by one, the last output
column ignored) land between 4.6e-3 and 26 on A-513, B-257 and C-128: each misses its case's
tolerance at least SEEDED_FACTOR = 100-fold (the smallest, A-513's dropped row, 415-fold) on
the restatement alone.

Adam criterion: test_dqn_train.py's teacher-forced T (1e-5 lr + ulp32(|x|)), derived there.

The fit that must learn (test_fit_learns_*): the Cornell box's radiance map at AREA_PER_SAMPLE
0.05 (474 volumes, 379 of them training rows: 3 Adam steps per epoch) after 2 frames of 64 x 64
at 4 spp, Glorot weights of seed 1984, batch 128, split seed 1984 at 0.8, FIT_EPOCHS = 60
epochs.  The fp64 restatement over the same schedule on the CPU restatement's map goes from a
first-epoch loss of 7330.30 (5074.04 after 5 epochs, 0.69 of it; half is first passed in epoch
47) to 3330.26 in epoch 60, 0.45 of it, at or below half: the schedule is long enough to
learn.  The device is only asked to end below its own first epoch.
"""
import functools

import numpy as np
import pytest

from test_dqn_train import LR, MARGIN, _HostAdam, _net, _ref, grad_error

RT_E_INVALID, RT_E_IO = -1, -4

GRAD_CASES = [("A", 1), ("A", 3), ("A", 64), ("A", 513),
              ("B", 1), ("B", 63), ("B", 64), ("B", 65), ("B", 128), ("B", 129), ("B", 257), ("B", 513),
              ("C", 128)]
UNCLIPPED = [("A", 3, True), ("A", 64, True)]
TOL_CASES = [(nm, n, False) for nm, n in GRAD_CASES] + UNCLIPPED
# 16 x the fp32 restatement's error (module docstring), never the device's
TOL = {
    "A-1": 7.5e-6, "A-3": 3.4e-6, "A-64": 6.0e-6, "A-513": 1.1e-5,
    "B-1": 1.1e-5, "B-63": 6.1e-6, "B-64": 5.9e-6, "B-65": 6.4e-6,
    "B-128": 7.8e-6, "B-129": 8.3e-6, "B-257": 9.5e-6, "B-513": 1.1e-5,
    "C-128": 6.8e-6, "A-3-unclipped": 3.8e-5, "A-64-unclipped": 5.8e-4,
}
SEEDED = [("A", 513), ("B", 257), ("C", 128)]
SEEDED_FACTOR = 100.0

ERR_CHUNK = 4096  # RT_DQN_FIT_ERROR_CHUNK
ERR_CASES = [("A", 1), ("A", 255), ("A", 256), ("A", 257), ("A", ERR_CHUNK + 1), ("B", 1), ("B", 257),
             ("B", ERR_CHUNK + 1)]
ERR_TOL = {
    "A-1": 6.5e-7, "A-255": 4.8e-8, "A-256": 6.1e-8, "A-257": 6.6e-8,
    "A-4097": 4.4e-8, "B-1": 1.2e-6, "B-257": 1.3e-6, "B-4097": 1.1e-6,
}

MAP_AREA = 0.05      # AREA_PER_SAMPLE of the small Cornell map
MAP_SEED = 1984
FIT_EPOCHS = 60


def _id(c):
    return f"{c[0]}-{c[1]}" + ("-unclipped" if len(c) > 2 and c[2] else "")


# --- restatements --------------------------------------------------------------

def _backward(d, hs, P):
    gW, gb = [None] * 4, [None] * 4
    for l in range(3, -1, -1):
        gW[l] = d.T @ hs[l]
        gb[l] = d.sum(0)
        if l > 0:
            d = (d @ P[l]) * (hs[l] > 0.0)
    return gW + gb


def dense_ref(ref, loc, tgt, mask=True, factor=2.0, col_weight=None):
    """(loss, [dW0..dW3, db0..db3]) of the dense step in fp64 on ref (an oracle.AdamRef).
    mask / factor / col_weight seed errors: no q > 0 mask, another factor, columns ignored."""
    hs = ref.forward(loc)
    q = hs[4]
    diff = np.asarray(tgt, np.float64).reshape(q.shape) - q
    if col_weight is not None:
        diff = diff * col_weight[None, :]
    loss = float(np.sum(diff * diff))
    d = -factor * diff
    if mask:
        d = np.where(q > 0.0, d, 0.0)
    return loss, _backward(d, hs, ref.P)


def _forward_f32(v, W, b, loc, order):
    f = np.float32
    if order == "numpy":
        mm = lambda a, c: a @ c
    elif order == "einsum":
        mm = lambda a, c: np.einsum("ik,kj->ij", a, np.ascontiguousarray(c))
    else:
        raise ValueError(order)
    v = np.asarray(v, f).ravel()
    W = [np.asarray(w, f) for w in W]
    b = [np.asarray(x, f).ravel() for x in b]
    loc = np.asarray(loc, f).reshape(-1, 3)
    hs = [v[None, :] - np.tile(loc, (1, v.size // 3))]
    for l in range(4):
        hs.append(np.maximum(mm(hs[l], W[l].T) + b[l][None, :], f(0)))
    return hs, W, mm


def dense_f32(v, W, b, loc, tgt, order="numpy"):
    """dense_ref in float32 with numpy alone: the yardstick of a correct fp32 dense step"""
    f = np.float32
    hs, W, mm = _forward_f32(v, W, b, loc, order)
    q = hs[4]
    diff = np.asarray(tgt, f).reshape(q.shape) - q
    loss = f(np.sum(diff * diff, dtype=f))
    d = np.where(q > 0, f(-2) * diff, f(0)).astype(f)
    gW, gb = [None] * 4, [None] * 4
    for l in range(3, -1, -1):
        gW[l] = mm(np.ascontiguousarray(d.T), hs[l])
        gb[l] = d.sum(0, dtype=f)
        if l > 0:
            d = (mm(d, W[l]) * (hs[l] > 0)).astype(f)
    return loss, gW + gb


def error_ref(ref, loc, tgt):
    q = ref.forward(loc)[4]
    diff = np.asarray(tgt, np.float64).reshape(q.shape) - q
    return float(np.sum(diff * diff))


def error_f32(v, W, b, loc, tgt, order="numpy"):
    q = _forward_f32(v, W, b, loc, order)[0][4]
    diff = (np.asarray(tgt, np.float32).reshape(q.shape) - q).astype(np.float64)
    return float(np.sum(diff * diff))


def fit_order_ref(oracle, seed, n, fraction):
    """rt_dqn_fit_order restated on oracle.philox"""
    key = [seed & 0xFFFFFFFF, seed >> 32]
    w = np.array([oracle.philox([i, 0, 0, 0x51466974], key) for i in range(n)], np.uint32).reshape(n, 4)
    u = ((w[:, 0] >> 8).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    train = u < np.float32(fraction)
    idx = np.arange(n)
    parts = []
    for sel in (train, ~train):
        i = idx[sel]
        parts.append(i[np.lexsort((i, w[sel, 1]))])
    return np.concatenate(parts).astype(np.int32), int(train.sum())


def _dense_adam(oracle, v, W, b):
    """oracle.AdamRef whose step is the dense one (the action argument is ignored)"""
    class DenseAdam(oracle.AdamRef):
        def loss_grads(self, loc, action, target):
            return dense_ref(self, loc, target)
    return DenseAdam(v, W, b, lr=LR)


def fit_ref_epochs(oracle, v, W, b, pos, q, seed, fraction, batch, epochs):
    """the fit's schedule in fp64: [(loss, error)] per epoch"""
    order, nt = fit_order_ref(oracle, seed, pos.shape[0], fraction)
    pos, q = pos[order], q[order]
    ad = _dense_adam(oracle, v, W, b)
    out = []
    for _ in range(epochs):
        loss = 0.0
        for b0 in range(0, nt, batch):
            b1 = min(b0 + batch, nt)
            loss += ad.step(pos[b0:b1], None, q[b0:b1])[0]
        out.append((loss, error_ref(ad, pos[nt:], q[nt:]) if nt < pos.shape[0] else 0.0))
    return out


# --- batches ---------------------------------------------------------------------

def _positions(name, n, rng):
    ref = _ref(name)
    cand = rng.uniform(-1, 1, (int(1.5 * n) + 64, 3)).astype(np.float32)
    margin = np.min([np.abs(z).min(axis=1) for z in ref.preactivations(cand)], axis=0)
    keep = np.nonzero(margin >= MARGIN)[0]
    assert keep.size >= n, (keep.size, n)
    return np.ascontiguousarray(cand[keep[:n]])


@functools.lru_cache(maxsize=None)
def _batch(name, n, unclipped=False):
    """dict(loc, tgt, loss, G, gn, q) by the module docstring's rule; cached and read-only"""
    ref = _ref(name)
    rng = np.random.default_rng(3000 + n)
    loc = _positions(name, n, rng)
    q = ref.forward(loc)[4]
    if unclipped:
        delta = rng.uniform(0.5, 1.0, q.shape) * rng.choice([-1.0, 1.0], q.shape)
        _, G = dense_ref(ref, loc, q + delta)
        delta *= 2.0 / np.sqrt(sum(float(np.sum(g * g)) for g in G))
        tgt = (q + delta).astype(np.float32)
    else:
        tgt = rng.uniform(0.0, 2.0, q.shape).astype(np.float32)
    loss, G = dense_ref(ref, loc, tgt)
    gn = float(np.sqrt(sum(float(np.sum(g * g)) for g in G)))
    assert np.count_nonzero(q > 0.0) >= 1, "at least one live output"
    if n >= 63:
        assert np.count_nonzero(q == 0.0) >= 3, "at least 3 dead outputs"
    for a in (loc, tgt):
        a.setflags(write=False)
    return dict(name=name, n=n, loc=loc, tgt=tgt, loss=loss, G=G, gn=gn, q=q)


@functools.lru_cache(maxsize=None)
def _fp32_errors(name, n, unclipped=False):
    bt = _batch(name, n, unclipped)
    v, W, b = _net(name)
    return tuple(grad_error(G, float(loss), bt["G"], bt["loss"])
                 for loss, G in (dense_f32(v, W, b, bt["loc"], bt["tgt"], order=o) for o in ("numpy", "einsum")))


@functools.lru_cache(maxsize=None)
def _err_batch(name, n):
    rng = np.random.default_rng(5000 + n)
    loc = _positions(name, n, rng)
    n_out = _ref(name).P[3].shape[0]
    tgt = rng.uniform(0.0, 2.0, (n, n_out)).astype(np.float32)
    for a in (loc, tgt):
        a.setflags(write=False)
    return dict(name=name, n=n, loc=loc, tgt=tgt, err=error_ref(_ref(name), loc, tgt))


@functools.lru_cache(maxsize=None)
def _err_fp32_errors(name, n):
    bt = _err_batch(name, n)
    v, W, b = _net(name)
    return tuple(abs(error_f32(v, W, b, bt["loc"], bt["tgt"], o) - bt["err"]) / bt["err"] for o in ("numpy", "einsum"))


def _seeded_errors(bt):
    """name -> (loss, gradients): the dense restatement with one error each"""
    ref, loc, tgt = _ref(bt["name"]), bt["loc"], np.asarray(bt["tgt"])
    n_out = tgt.shape[1]
    last_off = np.ones(n_out)
    last_off[-1] = 0.0
    return {
        "no q > 0 mask": dense_ref(ref, loc, tgt, mask=False),
        "factor 1 for 2": dense_ref(ref, loc, tgt, factor=1.0),
        "last row dropped": dense_ref(ref, loc[:-1], tgt[:-1]),
        "target columns rolled by one": dense_ref(ref, loc, np.roll(tgt, 1, axis=1)),
        f"column {n_out - 1} ignored": dense_ref(ref, loc, tgt, col_weight=last_off),
    }


# --- CPU: the split, the reader, the criterion ------------------------------------

@pytest.mark.parametrize("fraction", [0.8, 1.0])
@pytest.mark.parametrize("n", [1, 2, 5, 1000])
def test_fit_order_matches_the_philox_restatement(rtmi_mod, oracle_mod, n, fraction):
    for seed in (1984, (7 << 32) | 3):
        order, nt = rtmi_mod.dqn.fit_order(seed, n, fraction)
        want, want_nt = fit_order_ref(oracle_mod, seed, n, fraction)
        assert nt == want_nt and np.array_equal(order, want)
        assert np.array_equal(np.sort(order), np.arange(n))
        if fraction == 1.0:
            assert nt == n
        again, nt2 = rtmi_mod.dqn.fit_order(seed, n, fraction)
        assert nt2 == nt and np.array_equal(again, order)
    if n == 1000 and fraction == 0.8:
        assert 700 < nt < 900 and not np.array_equal(order[:nt], np.sort(order[:nt]))
        assert not np.array_equal(rtmi_mod.dqn.fit_order(1985, n, fraction)[0], order)


def test_fit_order_refuses_bad_fractions(rtmi_mod):
    for bad in (0.0, 1.5, float("nan"), -0.5):
        with pytest.raises(rtmi_mod.RtError) as e:
            rtmi_mod.dqn.fit_order(1984, 5, bad)
        assert e.value.code == RT_E_INVALID
    order, nt = rtmi_mod.dqn.fit_order(1984, 0, 0.8)
    assert order.size == 0 and nt == 0


def _write_table(path, pos, q):
    """a table in the save_q format; returns the float32 of every printed token"""
    lines, want = [str(q.shape[1])], []
    for p, row in zip(pos, q):
        toks = [f"{float(x):g}" for x in list(p) + list(row)]
        lines.append(" ".join(toks))
        want.append([np.float32(float(t)) for t in toks])
    path.write_text("\n".join(lines) + "\n")
    return np.array(want, np.float32).reshape(len(pos), 3 + q.shape[1]), lines


@pytest.mark.parametrize("rows,actions", [(3, 144), (1, 10)])
def test_qtable_read_returns_the_printed_tokens(rtmi_mod, tmp_path, rows, actions):
    import ctypes
    rng = np.random.default_rng(11)
    pos = rng.uniform(-1, 1, (rows, 3)).astype(np.float32)
    q = (rng.uniform(0, 3, (rows, actions)) * 10.0 ** rng.integers(-8, 3, (rows, actions))).astype(np.float32)
    want, _ = _write_table(tmp_path / "t.txt", pos, q)
    gp, gq = rtmi_mod.sarsa.read_q(str(tmp_path / "t.txt"))
    assert gp.shape == (rows, 3) and gq.shape == (rows, actions)
    assert np.array_equal(gp.view(np.uint32), want[:, :3].view(np.uint32))
    assert np.array_equal(gq.view(np.uint32), want[:, 3:].view(np.uint32))
    n, a = ctypes.c_int32(-1), ctypes.c_int32(-1)  # the sizing pass alone
    assert rtmi_mod.lib().rt_qtable_read(str(tmp_path / "t.txt").encode(), ctypes.byref(n), ctypes.byref(a),
                                         None, None) == 0
    assert (n.value, a.value) == (rows, actions)


def test_qtable_read_refuses_malformed_files(rtmi_mod, tmp_path):
    rng = np.random.default_rng(12)
    pos = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
    q = rng.uniform(0, 3, (3, 10)).astype(np.float32)
    _, lines = _write_table(tmp_path / "ok.txt", pos, q)
    assert rtmi_mod.sarsa.read_q(str(tmp_path / "ok.txt"))[1].shape == (3, 10)
    row3 = lines[2].split()
    bad = {
        "short": lines[:2] + [" ".join(row3[:-1])] + lines[3:],
        "long": lines[:2] + [" ".join(row3 + ["1.5"])] + lines[3:],
        "zero": ["0"] + lines[1:],
        "abc": lines[:2] + [" ".join(row3[:5] + ["abc"] + row3[6:])] + lines[3:],
    }
    for name, text in bad.items():
        p = tmp_path / f"{name}.txt"
        p.write_text("\n".join(text) + "\n")
        with pytest.raises(rtmi_mod.RtError) as e:
            rtmi_mod.sarsa.read_q(str(p))
        assert e.value.code == RT_E_IO, name
        assert ("line 1" if name == "zero" else "line 3") in str(e.value), (name, str(e.value))
    with pytest.raises(rtmi_mod.RtError) as e:
        rtmi_mod.sarsa.read_q(str(tmp_path / "missing.txt"))
    assert e.value.code == RT_E_IO


def test_batches_keep_the_margin_and_the_tables_are_complete(oracle_mod):
    assert sorted(TOL) == sorted(_id(c) for c in TOL_CASES)
    assert sorted(ERR_TOL) == sorted(_id(c) for c in ERR_CASES)
    for name, n, unc in TOL_CASES:
        bt = _batch(name, n, unc)
        zs = _ref(name).preactivations(bt["loc"])
        assert bt["loc"].shape == (n, 3) and min(float(np.abs(z).min()) for z in zs) >= MARGIN
        if unc:
            assert 0.05 <= bt["gn"] <= 2.5, bt["gn"]
        elif n >= 63:
            assert bt["gn"] > 10.0, bt["gn"]


@pytest.mark.parametrize("case", SEEDED, ids=_id)
def test_criterion_rejects_seeded_errors(oracle_mod, case):
    """On the restatement alone: each seeded error misses the case's tolerance at least
    SEEDED_FACTOR-fold, and the fp32 restatement in both orders is accepted."""
    bt = _batch(*case)
    tol = TOL[_id(case)]
    assert grad_error(bt["G"], bt["loss"], bt["G"], bt["loss"]) == 0.0
    for what, (loss, G) in _seeded_errors(bt).items():
        e = grad_error(G, loss, bt["G"], bt["loss"])
        print(f"{_id(case)} {what}: {e:.3g} = {e / tol:.3g} x tol")
        assert e > SEEDED_FACTOR * tol, (what, e, tol)
    for order, e in zip(("numpy", "einsum"), _fp32_errors(*case)):
        assert e <= tol, (order, e, tol)


@pytest.mark.parametrize("case", TOL_CASES, ids=_id)
def test_tolerances_are_16x_fp32_error(oracle_mod, case):
    tol = TOL[_id(case)]
    errs = _fp32_errors(*case)
    print(f"{_id(case)} fp32 numpy {errs[0]:.3g} einsum {errs[1]:.3g} tol {tol:.3g}")
    assert 16.0 * max(errs) <= tol <= 16.0 * max(errs) * 1.1 + 1e-12, (errs, tol)


@pytest.mark.parametrize("case", ERR_CASES, ids=_id)
def test_error_tolerances_are_16x_fp32_error(oracle_mod, case):
    tol = ERR_TOL[_id(case)]
    errs = _err_fp32_errors(*case)
    print(f"{_id(case)} fp32 numpy {errs[0]:.3g} einsum {errs[1]:.3g} tol {tol:.3g}")
    assert 16.0 * max(errs) <= tol <= 16.0 * max(errs) * 1.1 + 1e-12, (errs, tol)


def _epoch_rows():
    """test 8's data set: 300 synthetic rows for net A"""
    rng = np.random.default_rng(77)
    return rng.uniform(-1, 1, (300, 3)).astype(np.float32), rng.uniform(0, 2, (300, 10)).astype(np.float32)


def test_epoch_case_has_full_batches_and_a_ragged_one(rtmi_mod):
    _, nt = rtmi_mod.dqn.fit_order(1984, 300, 0.8)
    assert (nt + 127) // 128 >= 2 and nt % 128 != 0 and nt < 300
    assert rtmi_mod.dqn.fit_order(1984, 3, 1e-6)[1] == 0  # the split that leaves no training row


@functools.lru_cache(maxsize=None)
def _cornell(rtmi_mod):
    return rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU)


def _map_params(rtmi_mod):
    return rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=64, height=64, spp=4)


def test_the_schedule_learns_in_fp64(rtmi_mod, oracle_mod):
    """The condition on FIT_EPOCHS: the fp64 restatement over the device's schedule, on the
    CPU restatement's map, ends at or below half of its first-epoch loss."""
    g = _cornell(rtmi_mod)
    m = oracle_mod.Sarsa(g, MAP_SEED, MAP_AREA)
    m.render(oracle_mod.camera(rtmi_mod.CAMERAS["cornell"]), oracle_mod.params_from(_map_params(rtmi_mod)), 2)
    pos, q = m.volumes()[0], m.read()[0]
    assert 200 <= pos.shape[0] <= 999 and np.all(np.isfinite(q))
    W, b = rtmi_mod.dqn.glorot_weights(g.nn_vertices.size)
    hist = fit_ref_epochs(oracle_mod, g.nn_vertices, W, b, pos, q, 1984, 0.8, 128, FIT_EPOCHS)
    print(f"{pos.shape[0]} volumes; fp64 loss per epoch: {[round(l, 3) for l, _ in hist]}")
    assert hist[-1][0] <= 0.5 * hist[0][0], hist


# --- GPU -------------------------------------------------------------------------

def _dev(a, offset=0):
    """a on the device; offset: floats past a 16-byte boundary"""
    import torch
    a = np.array(a)
    if not offset:
        t = torch.from_numpy(a).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert buf.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 4 * offset
    return t


def _fit_step(tr, loc, tgt, offset=0):
    d_loc, d_tgt = _dev(loc), _dev(tgt, offset)
    return tr.fit_step_device(d_loc.data_ptr(), d_tgt.data_ptr(), len(loc))


def _trainer(rtmi_mod, gpu_ctx, name):
    v, W, b = _net(name)
    return rtmi_mod.dqn.DqnTrainer(gpu_ctx, v, W, b, learning_rate=LR)


def _bits(arrs):
    return [np.asarray(a, np.float32).view(np.uint32) for a in arrs]


def _same_bits(A, B):
    return all(np.array_equal(a, b) for a, b in zip(_bits(A), _bits(B)))


def _check_gradients(tr, bt, loss, gn, tol):
    G = sum(tr.grads(), [])
    e = grad_error(G, loss, bt["G"], bt["loss"])
    norm = float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in G)))
    print(f"{bt['name']}-{bt['n']}: grad_error {e:.3g} (tol {tol:.3g}), loss {loss:.9g} vs {bt['loss']:.9g}, "
          f"|g| {gn:.9g} vs read-out {norm:.9g}, reference {bt['gn']:.9g}")
    assert e <= tol, (e, tol)
    assert abs(gn - norm) <= 1e-5 * norm, (gn, norm)
    return G


@pytest.mark.gpu
@pytest.mark.parametrize("case", TOL_CASES, ids=_id)
def test_dense_step_element_by_element(rtmi_mod, oracle_mod, gpu_ctx, case):
    """One dense step of a fresh trainer: the loss, the norm and every gradient element."""
    bt = _batch(*case)
    with _trainer(rtmi_mod, gpu_ctx, case[0]) as tr:
        loss, gn = _fit_step(tr, bt["loc"], bt["tgt"])
        _check_gradients(tr, bt, loss, gn, TOL[_id(case)])
        assert (gn <= 5.0) if case[2] else (gn > 5.0 or case[1] < 63)


@pytest.mark.gpu
def test_dense_step_does_not_depend_on_the_targets_alignment(rtmi_mod, oracle_mod, gpu_ctx):
    """B at n = 65 with d_target one float past a 16-byte boundary (the scalar path) equals the
    aligned run (16-byte loads) bit for bit: loss, norm, gradients, parameters."""
    bt = _batch("B", 65)
    runs = []
    for offset in (0, 1):
        with _trainer(rtmi_mod, gpu_ctx, "B") as tr:
            out = _fit_step(tr, bt["loc"], bt["tgt"], offset)
            runs.append((out, sum(tr.grads(), []) + sum(tr.params(), [])))
    assert runs[0][0] == runs[1][0]
    assert _same_bits(runs[0][1], runs[1][1])
    assert grad_error(runs[1][1][:8], runs[1][0][0], bt["G"], bt["loss"]) <= TOL["B-65"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [("A", 3), ("A", 513), ("B", 65), ("B", 7300)])
def test_loss_kernel_alone_is_exact_in_its_gradient(rtmi_mod, oracle_mod, gpu_ctx, name, n):
    """rt_dqn_fit_loss_device on given q and targets: every dq element is numpy's float32
    q > 0 ? -2 (t - q) : 0 bit for bit (one rounding, in t - q), aligned or one float off; the
    loss, a float sum of `total` non-negative squares in another order, is within total x 2^-24
    of the double sum.  7300 rows of B are more quads than the 1024 x 256 threads of the grid."""
    import torch
    rng = np.random.default_rng(9000 + n)
    n_out = _ref(name).P[3].shape[0]
    q = np.maximum(rng.uniform(-0.5, 2.0, (n, n_out)), 0.0).astype(np.float32)  # a fifth dead
    t = rng.uniform(0.0, 2.0, (n, n_out)).astype(np.float32)
    diff = t - q
    want = np.where(q > 0, np.float32(-2) * diff, np.float32(0)).astype(np.float32)
    want_loss = float(np.sum(diff.astype(np.float64) ** 2))
    with _trainer(rtmi_mod, gpu_ctx, name) as tr:
        losses = []
        for offset in (0, 1):
            d_q, d_t = _dev(q), _dev(t, offset)
            d_dq = torch.full((n, n_out), float("nan"), dtype=torch.float32, device="cuda")
            losses.append(tr.fit_loss_device(d_q.data_ptr(), d_t.data_ptr(), n, d_dq.data_ptr()))
            assert np.array_equal(d_dq.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert losses[0] == losses[1]
        assert abs(losses[0] - want_loss) <= q.size * 2.0 ** -24 * want_loss


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("B", 257, False)] + UNCLIPPED, ids=_id)
def test_dense_adam_teacher_forced(rtmi_mod, oracle_mod, gpu_ctx, case):
    """Three dense steps, clipped and unclipped: every parameter equals the fp64 Adam
    recomputed from the device's own gradients (test_dqn_train.py's criterion)."""
    bt = _batch(*case)
    v, W, b = _net(case[0])
    host = _HostAdam(W, b)
    with _trainer(rtmi_mod, gpu_ctx, case[0]) as tr:
        for T in (1, 2, 3):
            loss, gn = _fit_step(tr, bt["loc"], bt["tgt"])
            if T == 1:  # (later steps leave the batch's own network: either branch, the host follows)
                assert (gn <= 5.0) if case[2] else (gn > 10.0)
            host.update(sum(tr.grads(), []), gn)
            w = host.worst(sum(tr.params(), []), T)
            print(f"step {T}: loss {loss:.6g} |g| {gn:.6g} worst {w:.3g} of the tolerance")
            assert w <= 1.0, (T, w)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("A", 0)] + ERR_CASES, ids=_id)
def test_fit_error_against_fp64(rtmi_mod, oracle_mod, gpu_ctx, case):
    name, n = case
    with _trainer(rtmi_mod, gpu_ctx, name) as tr:
        before = sum(tr.params(), [])
        if n == 0:
            assert tr.fit_error_device(0, 0, 0) == 0.0
            return
        bt = _err_batch(name, n)
        d_loc, d_tgt = _dev(bt["loc"]), _dev(bt["tgt"])
        e1 = tr.fit_error_device(d_loc.data_ptr(), d_tgt.data_ptr(), n)
        e2 = tr.fit_error_device(d_loc.data_ptr(), d_tgt.data_ptr(), n)
        rel = abs(e1 - bt["err"]) / bt["err"]
        print(f"{_id(case)}: error {e1!r} vs {bt['err']!r}: rel {rel:.3g} (tol {ERR_TOL[_id(case)]:.3g})")
        assert np.float64(e1).view(np.uint64) == np.float64(e2).view(np.uint64)
        assert rel <= ERR_TOL[_id(case)]
        assert _same_bits(before, sum(tr.params(), []))
        if name == "B":  # one float past a 16-byte boundary: the scalar path, the same sums
            d_off = _dev(bt["tgt"], 1)
            assert tr.fit_error_device(d_loc.data_ptr(), d_off.data_ptr(), n) == e1


@pytest.mark.gpu
def test_an_error_call_leaves_the_next_step_alone(rtmi_mod, oracle_mod, gpu_ctx):
    bt, eb = _batch("B", 257), _err_batch("B", 257)
    runs = []
    for with_error in (False, True):
        with _trainer(rtmi_mod, gpu_ctx, "B") as tr:
            if with_error:
                d_loc, d_tgt = _dev(eb["loc"]), _dev(eb["tgt"])
                tr.fit_error_device(d_loc.data_ptr(), d_tgt.data_ptr(), eb["n"])
            out = _fit_step(tr, bt["loc"], bt["tgt"])
            runs.append((out, sum(tr.grads(), []) + sum(tr.params(), [])))
    assert runs[0][0] == runs[1][0] and _same_bits(runs[0][1], runs[1][1])


@pytest.mark.gpu
def test_epoch_equals_its_steps(rtmi_mod, oracle_mod, gpu_ctx):
    """Net A, 300 rows, batch 128: one epoch() against the same slices fed by hand."""
    pos, q = _epoch_rows()
    order, nt = rtmi_mod.dqn.fit_order(1984, 300, 0.8)
    ps, qs = pos[order], q[order]
    with _trainer(rtmi_mod, gpu_ctx, "A") as tr, _trainer(rtmi_mod, gpu_ctx, "A") as hand:
        with rtmi_mod.dqn.QFit(gpu_ctx, tr, pos, q, seed=1984, train_fraction=0.8, batch_size=128) as fit:
            info = fit.info()
            assert info == {"n_train": nt, "n_test": 300 - nt, "n_batches": (nt + 127) // 128, "epochs_done": 0}
            assert info["n_batches"] >= 2 and nt % 128 != 0
            for ep in (1, 2):
                loss, err = fit.epoch()
                want = 0.0
                for b0 in range(0, nt, 128):
                    b1 = min(b0 + 128, nt)  # (the last batch ends where the training rows end)
                    want += _fit_step(hand, ps[b0:b1], qs[b0:b1])[0]
                d_loc, d_tgt = _dev(ps[nt:]), _dev(qs[nt:])
                want_err = hand.fit_error_device(d_loc.data_ptr(), d_tgt.data_ptr(), 300 - nt)
                assert _same_bits(sum(tr.params(), []), sum(hand.params(), []))
                assert loss == want and err == want_err and err > 0.0
                assert fit.info()["epochs_done"] == ep
    # a batch that holds every training row: one step per epoch
    with _trainer(rtmi_mod, gpu_ctx, "A") as tr, _trainer(rtmi_mod, gpu_ctx, "A") as hand:
        with rtmi_mod.dqn.QFit(gpu_ctx, tr, pos, q, batch_size=nt + 5) as fit:
            assert fit.info()["n_batches"] == 1
            loss, _ = fit.epoch()
        assert loss == _fit_step(hand, ps[:nt], qs[:nt])[0]
        assert _same_bits(sum(tr.params(), []), sum(hand.params(), []))
        # an empty test set is allowed: its error is 0
        with rtmi_mod.dqn.QFit(gpu_ctx, tr, pos, q, train_fraction=1.0) as fit:
            assert fit.info()["n_test"] == 0 and fit.epoch()[1] == 0.0


@pytest.mark.gpu
def test_fit_create_refuses_bad_data(rtmi_mod, oracle_mod, gpu_ctx):
    pos, q = _epoch_rows()
    with _trainer(rtmi_mod, gpu_ctx, "A") as tr:
        bad_q = q.copy()
        bad_q[17, 3] = np.nan
        inf_q = q.copy()
        inf_q[299, 9] = np.inf
        for args, kw in (((pos, q[:, :9]), {}), ((pos, bad_q), {}), ((pos, inf_q), {}),
                         ((pos[:3], q[:3]), {"train_fraction": 1e-6}), ((pos, q), {"batch_size": 0})):
            with pytest.raises(rtmi_mod.RtError) as e:
                rtmi_mod.dqn.QFit(gpu_ctx, tr, *args, **kw)
            assert e.value.code == RT_E_INVALID


@pytest.fixture(scope="module")
def cornell_map(rtmi_mod, gpu_ctx):
    """the small Cornell radiance map after 2 frames: (geometry, scene, map, pos, q)"""
    g = _cornell(rtmi_mod)
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        rm = rtmi_mod.sarsa.RadianceMap(gpu_ctx, sc, MAP_SEED, area_per_sample=MAP_AREA)
        try:
            rm.render(rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"]), _map_params(rtmi_mod), 2)
            yield g, sc, rm, rm.volumes()[0], rm.read()[0]
        finally:
            rm.close()


def _glorot_trainer(rtmi_mod, gpu_ctx, g):
    W, b = rtmi_mod.dqn.glorot_weights(g.nn_vertices.size)
    return rtmi_mod.dqn.DqnTrainer(gpu_ctx, g.nn_vertices, W, b, learning_rate=LR)


@pytest.mark.gpu
def test_fit_from_a_map_and_from_a_file(rtmi_mod, oracle_mod, gpu_ctx, cornell_map, tmp_path):
    g, sc, rm, pos, q = cornell_map
    assert 200 <= pos.shape[0] <= 999 and q.shape == (pos.shape[0], 144)
    assert np.unique(q).size > 10  # a learned table, not the initial constant
    path = str(tmp_path / "radiance_map_data.txt")
    rm.save_q(path)
    fpos, fq = rtmi_mod.sarsa.read_q(path)
    assert fq.shape == q.shape and np.allclose(fq, q, rtol=1e-5, atol=1e-7)
    results = []
    for make in (lambda tr: rtmi_mod.dqn.QFit.from_map(gpu_ctx, tr, rm),
                 lambda tr: rtmi_mod.dqn.QFit(gpu_ctx, tr, pos, q),
                 lambda tr: rtmi_mod.dqn.QFit.from_file(gpu_ctx, tr, path),
                 lambda tr: rtmi_mod.dqn.QFit(gpu_ctx, tr, fpos, fq)):
        with _glorot_trainer(rtmi_mod, gpu_ctx, g) as tr, make(tr) as fit:
            results.append((fit.epoch(), sum(tr.params(), [])))
    for a, c in ((0, 1), (2, 3)):
        assert results[a][0] == results[c][0] and _same_bits(results[a][1], results[c][1])
    assert np.array_equal(rm.read()[0].view(np.uint32), q.view(np.uint32))


@pytest.mark.gpu
def test_fit_learns_and_the_result_renders(rtmi_mod, oracle_mod, gpu_ctx, cornell_map):
    """FIT_EPOCHS epochs from Glorot weights (module docstring): the last epoch's loss is below
    the first's; the fitted parameters in the bf16 inference network agree with the restated
    bf16 forward within tests/test_dqn.py's tolerances for that comparison."""
    g, sc, rm, pos, q = cornell_map
    with _glorot_trainer(rtmi_mod, gpu_ctx, g) as tr:
        with rtmi_mod.dqn.QFit.from_map(gpu_ctx, tr, rm) as fit:
            hist = [fit.epoch() for _ in range(FIT_EPOCHS)]
            order, nt = rtmi_mod.dqn.fit_order(1984, pos.shape[0], 0.8)
            assert fit.info() == {"n_train": nt, "n_test": pos.shape[0] - nt, "n_batches": (nt + 127) // 128,
                                  "epochs_done": FIT_EPOCHS}
        print("device (loss, error) per epoch:", [(round(l, 3), round(e, 3)) for l, e in hist])
        assert all(np.isfinite(l) and np.isfinite(e) for l, e in hist)
        assert hist[-1][0] < hist[0][0]
        W, b = tr.params()
    pts = pos[order[:16]]
    with rtmi_mod.dqn.Dqn(gpu_ctx, g.nn_vertices, W, b) as net:
        got = net.forward(pts)
    qe = oracle_mod.dqn_forward(W, b, g.nn_vertices, pts, bf16=True)
    err = np.abs(got - qe)
    assert np.abs(qe).max() > 0.0
    assert err.max() <= 2e-2 * np.abs(qe).max() + 1e-6, err.max()
    assert err.mean() <= 2e-3 * np.abs(qe).mean() + 1e-7, err.mean()
