"""Training on PUCT visit targets, CPU side: the numpy restatement of the target
(tests/pi_ref.py) tied to the planes-consistent label map, the new entry points' argument
checks (no GPU needed) and the CPU trainer on soft targets."""
import ctypes

import numpy as np
import torch

import pi_ref
import training
from gzero import _lib

GZ_ERR_ARG = -1


def test_one_hot_rows_follow_the_fixed_label_map():
    """A one-hot visit row at cell c moves to the one-hot row at the planes-consistent
    label of c (training._transform_index(fix_labels=True), pinned to the planes by
    test_oracle_fixed_labels_follow_planes), for every cell and all 8 symmetries."""
    for c in range(225):
        row = np.zeros(225, np.uint16)
        row[c] = 7
        for k in range(4):
            for flip in (False, True):
                want = np.zeros(225, np.float32)
                want[training._transform_index(c, k, flip, fix_labels=True)] = 1.0
                assert np.array_equal(pi_ref.pi_sample(row, k, flip), want), (c, k, flip)


def test_pi_dataset_numbering_and_nan_rows():
    rng = np.random.default_rng(5)
    vis = rng.integers(0, 50, (3, 225)).astype(np.uint16)
    vis[1] = 0
    sel = [2, 7]  # 7: a selection out of range
    pi = pi_ref.pi_dataset(vis, sel)
    assert pi.shape == (3 + 16, 225) and pi.dtype == np.float32
    assert np.array_equal(pi[0], vis[0].astype(np.float32) / np.float32(vis[0].sum()))
    assert np.isnan(pi[1]).all() and np.isnan(pi[3 + 8:]).all()
    assert np.array_equal(pi[3 + 2 * 1 + 1], pi_ref.pi_sample(vis[2], 1, True))
    assert np.isnan(pi_ref.pi_dataset(vis, sel, [-1, 19])).all()


def test_soft_entry_points_check_arguments_without_gpu():
    L = _lib.load()
    buf = (ctypes.c_float * 225)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.gz_dataset_pi(p, -1, None, 0, None, 0, p, None) == GZ_ERR_ARG
    assert b"gz_dataset_pi" in L.gz_last_error()
    assert L.gz_dataset_pi(p, 1, None, 0, None, 1, None, None) == GZ_ERR_ARG
    assert L.gz_dataset_pi(None, 0, p, 1, None, 8, p, None) == GZ_ERR_ARG  # augmenting an empty replay
    assert b"empty replay" in L.gz_last_error()
    assert L.gz_dataset_pi(p, 1, None, 0, None, 0, None, None) == _lib.GZ_OK  # nothing to do
    fc = _lib.SgdFc(*[p.value] * 6)
    args = lambda B, pi: (ctypes.byref(fc), B, p, p, pi, p, 1.0, p, p, ctypes.byref(fc), p, p, None)  # noqa: E731
    assert L.gz_sgd_fc_loss_soft(*args(0, p)) == GZ_ERR_ARG
    assert b"gz_sgd_fc_loss_soft" in L.gz_last_error()
    assert L.gz_sgd_fc_loss_soft(*args(1, None)) == GZ_ERR_ARG


class _TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Linear(675, 225)
        self.v = torch.nn.Linear(675, 1)

    def forward(self, x):
        f = x.reshape(x.shape[0], -1)
        return self.p(f), torch.tanh(self.v(f))


class _SoftSet:
    soft = True

    def __init__(self, x, pi, v):
        self.x, self.pi, self.v = x, pi, v

    def __len__(self):
        return len(self.v)

    def gather(self, ids):
        return self.x[ids], self.pi[ids], self.v[ids]


def test_cpu_trainer_takes_soft_targets():
    """DeviceTrainer(device="cpu") (torch's modules under autograd) on probability
    targets: one epoch trains (the parameters move) and validates, to finite losses."""
    from gzero.train import DeviceTrainer
    g = torch.Generator().manual_seed(3)
    n = 200
    x = (torch.rand((n, 3, 15, 15), generator=g) < 0.3).float()
    counts = torch.zeros((n, 225))
    for i in range(n):
        cells = torch.randperm(225, generator=g)[:12]
        draws = cells[torch.randint(0, 12, (50,), generator=g)]
        counts[i] = torch.bincount(draws, minlength=225).float()
    pi = counts / counts.sum(1, keepdim=True)
    v = torch.randint(-1, 2, (n, 1), generator=g).float()
    ds = _SoftSet(x, pi, v)
    torch.manual_seed(0)
    tr = DeviceTrainer(_TinyNet(), device="cpu")
    before = [p.detach().clone() for p in tr.net.parameters()]
    tl = tr.train_epoch(ds, batch_size=64)
    vl = tr.validate_epoch(ds, batch_size=64)
    assert np.isfinite(tl) and np.isfinite(vl)
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.net.parameters()))
