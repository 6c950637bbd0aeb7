"""Plain numpy / torch-float64 restatement of the visit-distribution training target
(include/gzero.h: gz_dataset_pi, gz_sgd_fc_loss_soft), the checker of tests/test_pi_cpu.py
and tests/test_gpu_pi.py.

* ``pi_sample(row, k, flip)``: the row of visit counts moved exactly as the planes are
  (training._transform_planes: np.rot90 counter-clockwise k times, then the horizontal
  flip), divided in float32 by its sum.  A row whose sum is 0 gives NaN.
* ``pi_dataset(visits, sel, ids)``: the samples of GomokuSelfPlayDataset's numbering
  (originals, then 8 per selected record in (k, flip) order); an id or a selection out of
  range gives a row of NaN.
* ``soft_loss(...)``: CrossEntropy with probability targets + MSE on the FC heads and its
  gradients by torch autograd in float64.
"""
import numpy as np
import torch
import torch.nn as nn

import training


def pi_sample(row, k=0, flip=False):
    row = np.asarray(row, np.uint16)
    moved = training._transform_planes(row.reshape(1, 15, 15), k, flip).reshape(225)
    s = int(row.sum())
    if s == 0:
        return np.full(225, np.nan, np.float32)
    return moved.astype(np.float32) / np.float32(s)


def pi_dataset(visits, sel, ids=None):
    visits = np.asarray(visits, np.uint16).reshape(-1, 225)
    n, m = len(visits), len(sel)
    ids = range(n + 8 * m) if ids is None else ids
    out = np.full((len(ids), 225), np.nan, np.float32)
    for o, s in enumerate(ids):
        s = int(s)
        if not 0 <= s < n + 8 * m:
            continue
        rec, k, flip = (s, 0, False) if s < n else (int(sel[(s - n) >> 3]), ((s - n) & 7) >> 1, bool((s - n) & 1))
        if 0 <= rec < n:
            out[o] = pi_sample(visits[rec], k, flip)
    return out


def soft_loss(fcs, pin, vin, pi, v, scale=1.0):
    """fcs = (policy_fc.weight, .bias, value_fc1.weight, .bias, value_fc2.weight, .bias); all
    arguments tensors (any device / dtype).  Returns ((loss, ce, mse) floats, [dL/dpin,
    dL/dvin, the six FC gradients] float64 CPU tensors), the gradients of scale * loss."""
    ref = [t.detach().double().cpu().requires_grad_() for t in fcs]
    p64 = pin.detach().double().cpu().requires_grad_()
    v64 = vin.detach().double().cpu().requires_grad_()
    B = p64.shape[0]
    lg = p64 @ ref[0].T + ref[1]
    val = torch.tanh(torch.relu(v64 @ ref[2].T + ref[3]) @ ref[4].T + ref[5])
    ce = nn.CrossEntropyLoss()(lg, pi.detach().double().cpu())
    mse = nn.MSELoss()(val, v.detach().double().cpu().view(B, 1))
    ((ce + mse) * scale).backward()
    loss = [float(t.detach()) for t in (ce + mse, ce, mse)]
    return tuple(loss), [p64.grad, v64.grad] + [r.grad for r in ref]
