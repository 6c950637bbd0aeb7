"""Training on PUCT visit targets on the GPU: gz_dataset_pi (csrc/gz_train.hip) bit for bit
against the numpy restatement (tests/pi_ref.py), gz_sgd_fc_loss_soft (csrc/gz_sgd.hip)
against torch autograd in float64 and, for one-hot rows, bit for bit against the hard-label
gz_sgd_fc_loss, and the soft step through gzero.sgd.NetStep / gzero.train.DeviceDataset.

Tolerances are those of tests/test_gpu_sgd.py for the hard-label step (the same
arithmetic plus one 225-term sum): the loss within 1e-6 relative, every gradient within
1e-5 of the float64 gradient's norm (relative Frobenius error)."""
import ctypes
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import SEED
import pi_ref

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- gz_dataset_pi


def _visit_rows():
    """n = 5 rows of counts.  A row's non-zero counts are pairwise distinct and sit on
    random cells (225 distinct counts would sum to 25,200 > 4095), so a row equals none
    of its 7 other symmetries; the sums are 1830, 4095 (the largest a search can give), 1
    (the smallest), 465 and 153."""
    rng = np.random.default_rng(SEED)
    vis = np.zeros((5, 225), np.uint16)
    for r, k in enumerate((60, 80, 1, 30, 17)):
        vis[r, rng.choice(225, k, replace=False)] = rng.permutation(np.arange(1, k + 1))
    vis[1, np.argmax(vis[1])] += 4095 - int(vis[1].sum())
    assert [int(s) for s in vis.sum(1)] == [1830, 4095, 1, 465, 153]
    return vis


SEL = [3, 0]


def _pi(vis, sel, ids, count=None, fill=None):
    """gz_dataset_pi on device copies; ids None = the whole-set build."""
    from gzero import _lib
    L = _lib.load()
    n, m = len(vis), len(sel)
    count = (n + 8 * m if ids is None else len(ids)) if count is None else count
    d_vis = torch.from_numpy(np.ascontiguousarray(vis).view(np.int16)).cuda()
    d_sel = torch.tensor(sel if sel else [0], dtype=torch.int32, device="cuda")
    d_ids = None if ids is None else torch.tensor(list(ids), dtype=torch.int64, device="cuda")
    # one guard row behind the output: the kernel must not write past `count` rows
    out = torch.full((count + 1, 225), -7.0 if fill is None else fill, dtype=torch.float32, device="cuda")
    _lib.check(L.gz_dataset_pi(_ptr(d_vis), n, _ptr(d_sel), m, _ptr(d_ids), count, _ptr(out), _stream()),
               "gz_dataset_pi")
    got = out.cpu().numpy()
    assert (got[count] == (-7.0 if fill is None else fill)).all()
    return got[:count]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_dataset_pi_whole_set_exact():
    vis = _visit_rows()
    got = _pi(vis, SEL, None)
    want = pi_ref.pi_dataset(vis, SEL)
    assert got.shape == (21, 225) and np.isfinite(want).all()
    assert _same_bits(got, want)
    # every one of the 8 symmetries of a selected row is a different row
    assert len({got[5 + j].tobytes() for j in range(8)}) == 8


@pytest.mark.parametrize("count", [1, 21, 300])
def test_dataset_pi_gather_exact(count):
    """Permuted ids with duplicates; 300 samples cross a 256-thread workgroup whatever
    the thread-to-sample mapping."""
    vis = _visit_rows()
    rng = np.random.default_rng(SEED + count)
    ids = [int(i) for i in rng.integers(0, 21, count)]
    if count == 21:
        ids = [int(i) for i in rng.permutation(21)]
        ids[4] = ids[11]
    assert _same_bits(_pi(vis, SEL, ids), pi_ref.pi_dataset(vis, SEL, ids))


def test_dataset_pi_nan_rows():
    """An id outside [0, n + 8m), a selection outside [0, n) and a row whose sum is 0 give
    NaN rows; their neighbours stay intact."""
    vis = _visit_rows()
    ids = [20, 21, 0, -1, 6, 2 ** 40, 13]
    got = _pi(vis, SEL, ids)
    want = pi_ref.pi_dataset(vis, SEL, ids)
    assert [bool(np.isnan(r).all()) for r in got] == [False, True, False, True, False, True, False]
    assert not np.isnan(got[[0, 2, 4, 6]]).any()
    assert _same_bits(got[[0, 2, 4, 6]], want[[0, 2, 4, 6]])
    vis[2] = 0
    for sel in ([3, 0], [2, 5], [-1, 4]):  # row 2 is empty; 5 and -1 are no rows
        got = _pi(vis, sel, None)
        want = pi_ref.pi_dataset(vis, sel)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(got[2]).all() and not np.isnan(got[[0, 1, 3, 4]]).any()
        assert _same_bits(np.nan_to_num(got, nan=-1.0), np.nan_to_num(want, nan=-1.0))
    assert np.isnan(_pi(vis, [2, 5], None)[5:]).all()
    assert _pi(vis, SEL, [], count=0).shape == (0, 225)


def test_one_hot_rows_follow_the_fixed_labels():
    """DeviceDataset(visits=...) next to the hard dataset on the same records, selection
    and ids: with one-hot rows at each record's move, argmax(pi) is the label
    gz_dataset_gather gives with GZ_AUG_FIX_LABELS, and pi is exactly one-hot; the planes
    and values are the hard dataset's."""
    from gzero.boards import RECORD_DTYPE, cells_to_words
    from gzero.train import DeviceDataset
    rng = np.random.default_rng(SEED + 1)
    n = 5
    cells = rng.choice(np.array([0, 0, 0, 1, 2], np.int8), size=(n, 225))
    rec = np.zeros(n, RECORD_DTYPE)
    rec["black"], rec["white"] = cells_to_words(cells)
    rec["move"] = rng.choice(225, n, replace=False)
    rec["z"] = rng.integers(-1, 2, n)
    vis = np.zeros((n, 225), np.uint16)
    vis[np.arange(n), rec["move"]] = 8
    hard = DeviceDataset(rec, augment_ratio=0.5, fix_labels=True, rng=random.Random(4))
    soft = DeviceDataset(rec, augment_ratio=0.5, fix_labels=True, rng=random.Random(4), visits=vis)
    assert soft.soft and not hard.soft and len(soft) == len(hard) == n + 16
    ids = torch.tensor([int(i) for i in rng.permutation(len(soft))] + [3, 3], dtype=torch.int64, device="cuda")
    x0, y0, v0 = hard.gather(ids)
    x1, pi, v1 = soft.gather(ids)
    assert pi.dtype == torch.float32 and tuple(pi.shape) == (len(ids), 225)
    assert torch.equal(x0, x1) and torch.equal(v0, v1)
    assert torch.equal(pi.argmax(1), y0)
    assert torch.equal(pi, nn.functional.one_hot(y0, 225).float())
    # the whole set and single samples go through the same kernel
    xa, pa, va = soft.materialize()
    assert torch.equal(pa[ids], pi) and torch.equal(xa[ids], x1) and torch.equal(va[ids], v1)
    xi, pi_i, vi = soft[n + 5]
    assert torch.equal(pi_i, pa[n + 5]) and torch.equal(xi, xa[n + 5]) and tuple(pi_i.shape) == (225,)
    # a device tensor of counts is taken as it is
    dev = DeviceDataset(rec, augment_ratio=0.5, fix_labels=True, rng=random.Random(4),
                        visits=torch.from_numpy(vis.view(np.int16)).cuda())
    assert torch.equal(dev.gather(ids)[1], pi)
    with pytest.raises(ValueError):
        DeviceDataset(rec, visits=vis[:3])


# ---------------------------------------------------------------- gz_sgd_fc_loss_soft


def _net(seed):
    from gzero import weights
    net = weights.PolicyValueNet()
    net.load_state_dict(weights.init_state_dict(seed))
    return net


def _sparse_pi(B, seed):
    """Normalised multinomial counts of 200 draws over a random subset of cells: sparse
    rows, like the visit rows of a search."""
    rng = np.random.default_rng(seed)
    pi = np.zeros((B, 225), np.float32)
    for b in range(B):
        cells = rng.choice(225, int(rng.integers(3, 40)), replace=False)
        counts = rng.multinomial(200, rng.dirichlet(np.ones(len(cells))))
        pi[b, cells] = counts.astype(np.float32) / np.float32(200)
    return torch.from_numpy(pi)


_FC_CACHE = {}


def _fc_inputs(B):
    """The heads' inputs and weights of a case, made once and left unchanged."""
    if B not in _FC_CACHE:
        g = torch.Generator().manual_seed(SEED + B)
        net = _net(SEED + 3).cuda()
        fcs = [net.policy_fc.weight, net.policy_fc.bias, net.value_fc1.weight, net.value_fc1.bias,
               net.value_fc2.weight, net.value_fc2.bias]
        _FC_CACHE[B] = ([t.detach() for t in fcs], (torch.randn(B, 450, generator=g) * 0.5).cuda(),
                        (torch.randn(B, 225, generator=g) * 0.5).cuda(), (torch.rand(B, generator=g) * 2 - 1).cuda())
    return _FC_CACHE[B]


def _fc_loss(soft, fcs, pin, vin, target, v, scale, fill=NAN):
    """gz_sgd_fc_loss / gz_sgd_fc_loss_soft into pre-filled buffers -> [loss[3], dpin, dvin,
    the six FC gradients] (eleven outputs counting the loss slots)."""
    from gzero import _lib
    L = _lib.load()
    B = pin.shape[0]
    grads = [torch.full_like(t, fill) for t in fcs]
    dpin, dvin = torch.full_like(pin, fill), torch.full_like(vin, fill)
    loss = torch.full((3,), fill, device="cuda")
    ws = torch.empty(int(L.gz_sgd_fc_workspace_bytes(B)), dtype=torch.uint8, device="cuda")
    fc, fcg = _lib.SgdFc(*[t.data_ptr() for t in fcs]), _lib.SgdFc(*[t.data_ptr() for t in grads])
    fn, who = (L.gz_sgd_fc_loss_soft, "gz_sgd_fc_loss_soft") if soft else (L.gz_sgd_fc_loss, "gz_sgd_fc_loss")
    target = target.cuda().contiguous()
    _lib.check(fn(ctypes.byref(fc), B, _ptr(pin), _ptr(vin), _ptr(target), _ptr(v), scale, _ptr(dpin), _ptr(dvin),
                  ctypes.byref(fcg), _ptr(loss), _ptr(ws), _stream()), who)
    torch.cuda.synchronize()
    return [loss, dpin, dvin] + grads


def _check_vs_float64(out, fcs, pin, vin, pi, v, scale):
    want, grads = pi_ref.soft_loss(fcs, pin, vin, pi, v, scale)
    got = out[0].double().cpu()
    errs = []
    for a, b in zip(got, want):
        print("loss", float(a), b)
        assert abs(float(a) - b) <= 1e-6 * max(1.0, abs(b)), (float(a), b)
    for k, (a, b) in enumerate(zip(out[1:], grads)):
        err = float((a.double().cpu() - b).norm()) / max(float(b.norm()), 1e-30)
        errs.append(err)
    print("relative Frobenius errors", ["%.2e" % e for e in errs])
    assert max(errs) < 1e-5, errs


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("B", [1, 7, 17, 128, 65, 130])
def test_soft_loss_vs_float64(B, scale):
    """17 boards are one more than the gemm's 16-row tile; 65 and 130 are one and two
    more than the 64 boards a wave's lanes take at a time, and 130 is above 128."""
    fcs, pin, vin, v = _fc_inputs(B)
    pi = _sparse_pi(B, SEED + 7 * B)
    assert float((pi.sum(1) - 1).abs().max()) < 1e-6
    _check_vs_float64(_fc_loss(True, fcs, pin, vin, pi, v, scale), fcs, pin, vin, pi, v, scale)


@pytest.mark.parametrize("B", [7, 128])
def test_unnormalised_rows_vs_float64(B):
    """torch's CrossEntropyLoss takes any non-negative row as it is: rows that sum to 2."""
    fcs, pin, vin, v = _fc_inputs(B)
    pi = 2.0 * _sparse_pi(B, SEED + 7 * B)
    _check_vs_float64(_fc_loss(True, fcs, pin, vin, pi, v, 1.0), fcs, pin, vin, pi, v, 1.0)


@pytest.mark.parametrize("B,scale", [(7, 0.25), (128, 1.0), (65, 1.0)])
def test_one_hot_rows_equal_the_hard_path_bitwise(B, scale):
    fcs, pin, vin, v = _fc_inputs(B)
    y = torch.randint(0, 225, (B,), generator=torch.Generator().manual_seed(SEED + B))
    hard = _fc_loss(False, fcs, pin, vin, y, v, scale)
    soft = _fc_loss(True, fcs, pin, vin, nn.functional.one_hot(y, 225).float(), v, scale)
    assert len(hard) == len(soft) == 9 and hard[0].numel() == 3  # eleven outputs
    for k, (a, b) in enumerate(zip(hard, soft)):
        assert not torch.isnan(a).any(), k
        assert torch.equal(a, b), (k, float((a - b).abs().max()))


@pytest.mark.parametrize("bad", [-0.1, NAN])
def test_bad_rows_poison_the_step(bad):
    """One entry below 0 (or not finite) in one row: the loss and the mean cross-entropy
    are NaN and every gradient tensor is poisoned, as by a label outside [0, 225).  The
    NaN enters through that board's scale/B factor, exactly as on the hard path, so it
    reaches: all of dL/dW and dL/db of policy_fc and value_fc2, that board's rows of
    dL/dpin and dL/dvin, and the rows of value_fc1's gradients whose unit is active on
    that board (ReLU passes no gradient, NaN or not, through an inactive unit).  The other
    boards' rows of dL/dpin and dL/dvin are written and finite.  Buffers are pre-filled
    with 0.25, so an output that was not written cannot pass for NaN."""
    B, row = 7, 4
    fcs, pin, vin, v = _fc_inputs(B)
    pi = _sparse_pi(B, SEED + 7 * B)
    good = _fc_loss(True, fcs, pin, vin, pi, v, 1.0, fill=0.25)
    pi[row, int(torch.nonzero(pi[row])[0])] = bad
    loss, dpin, dvin, gpw, gpb, g1w, g1b, g2w, g2b = _fc_loss(True, fcs, pin, vin, pi, v, 1.0, fill=0.25)
    assert torch.isnan(loss[0]) and torch.isnan(loss[1])
    assert torch.equal(loss[2], good[0][2])  # the squared error has no cross-entropy in it
    for k, t in enumerate((dpin, dvin, gpw, gpb, g1w, g1b, g2w, g2b)):
        assert torch.isnan(t).any(), k
    for t in (gpw, gpb, g2w, g2b, dpin[row], dvin[row]):
        assert torch.isnan(t).all()
    others = [b for b in range(B) if b != row]
    assert torch.equal(dpin[others], good[1][others]) and torch.equal(dvin[others], good[2][others])
    active = (vin[row] @ fcs[2].T + fcs[3]) > 1e-4  # units clearly on the active side
    assert active.any() and torch.isnan(g1b[active]).all() and torch.isnan(g1w[active]).all()


# ---------------------------------------------------------------- NetStep on soft targets


def _planes(B, seed):
    rng = np.random.default_rng(seed)
    cells = rng.choice(np.array([0, 0, 0, 1, 2], np.int8), size=(B, 225))
    x = np.stack([cells == 1, cells == 2, cells == 0], 1).reshape(B, 3, 15, 15).astype(np.float32)
    v = rng.uniform(-1, 1, (B, 1)).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda()


def test_netstep_soft_matches_the_autograd_path():
    """NetStep.step with probability targets against sgd.train_forward + F.cross_entropy(
    logits, pi) + MSE under autograd (the same tower kernels): the bounds of
    test_netstep_matches_the_autograd_path -- loss within 1e-6 relative, every gradient
    within 1e-5 (relative Frobenius; or below 1e-6 of the largest gradient norm for the
    conv biases whose gradient is zero), buffers identical."""
    from gzero import sgd
    B = 128
    x, v = _planes(B, SEED + 21)
    pi = _sparse_pi(B, SEED + 22).cuda()
    nets = [_net(SEED + 4).cuda(), _net(SEED + 4).cuda()]
    step = sgd.NetStep(nets[0])
    nets[0].train()
    l0 = float(step.step(x, pi, v))
    nets[1].train()
    lg, val = sgd.train_forward(nets[1], x)
    loss = nn.functional.cross_entropy(lg, pi) + nn.MSELoss()(val, v)
    loss.backward()
    ref = float(loss.detach())
    print("loss", l0, ref)
    assert abs(l0 - ref) <= 1e-6 * abs(ref)
    top = max(float(p.grad.norm()) for p in nets[1].parameters())
    for (k, a), (_, b) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        err = float((a.grad - b.grad).norm()) / max(float(b.grad.norm()), 1e-30)
        assert err < 1e-5 or float((a.grad - b.grad).norm()) < 1e-6 * top, (k, err)
    for (k, a), (_, b) in zip(nets[0].named_buffers(), nets[1].named_buffers()):
        assert torch.equal(a, b), k
    # the target's kind picks the kernel; anything else is refused
    for y in (pi[:, :200], pi[0], torch.zeros((B, 225), dtype=torch.int64, device="cuda"),
              torch.zeros(B, device="cuda"), torch.zeros(B, dtype=torch.bool, device="cuda")):
        with pytest.raises(ValueError):
            step.step(x, y, v)


def test_soft_steps_learn_the_distribution():
    """One fixed batch of 64 soft samples, 20 NetStep + DeviceAdam steps at the trainer's
    defaults: the soft cross-entropy falls, and at every step it is at least the batch's
    mean entropy -sum pi log pi minus 1e-5 (Gibbs' inequality)."""
    from gzero.train import DeviceTrainer
    B = 64
    x, v = _planes(B, SEED + 31)
    pi = _sparse_pi(B, SEED + 32)
    p64 = pi.double()
    entropy = float(-(p64 * torch.log(p64.clamp_min(1e-300))).sum(1).mean())
    tr = DeviceTrainer(_net(SEED + 5))
    tr.net.train()
    pi = pi.cuda()
    ces = []
    for _ in range(20):
        tr.step_fn.step(x, pi, v)
        ces.append(tr.step_fn.loss[1].clone())
        tr.clip_and_step()
    ces = [float(c) for c in torch.stack(ces).cpu()]
    print("entropy", entropy, "soft cross-entropy", ces[0], "->", ces[-1])
    assert all(np.isfinite(c) and c >= entropy - 1e-5 for c in ces), (entropy, ces)
    assert ces[-1] < ces[0], ces
