"""gz_pv_forward(GZ_PV_F16) on the GPU against its CPU restatement (tests/pv_f16_ref.py).

Accuracy.  For every weight set the two CPU evaluations of the specification give, per
output (logits, value, softmax):
    E = max |emu64 - fp64 torch|   what the fp16 maps and weights cost,
    D = max |emu32 - emu64|        how far two correct evaluations of the same
                                   specification land from each other (fp16 rounding-
                                   boundary flips caused by accumulation rounding).
The kernel is a third accumulation order, so it must lie
    1. within 4 D of emu64 (4: the tail of a maximum over ~58 k values; an implementation
       that drops or adds a rounding point lands ~E away, which is more),
    2. within E + 4 D of the fp64 network,
    3. at least E / 4 away from the f16x3 forward on the logits (it is not f16x3 under
       another name).
The bounds come from the CPU references alone, never from the kernel.

Shapes: n = 1, n = 7, n = CUs + 3 (a workgroup runs a second board on the LDS its first
one left: the zero slots, and no lo plane), d_count < n; batch invariance with ==; the
f16x3 forward byte-identical before and after an F16 call on the same workspace."""
import numpy as np
import pytest
import torch

import pv_f16_ref as F
from gzero import _lib, boards, device, weights

pytestmark = pytest.mark.gpu

_REF, _GPU, _W = {}, {}, {}


def _n_boards():
    return torch.cuda.get_device_properties(0).multi_processor_count + 3  # 259 on the MI355X


def _cells():
    return F.board_cells(_n_boards(), seed=0)


def _rows(cells):
    bl, wh = boards.cells_to_words(cells)
    return boards.leaf_words(bl, wh)


def _sd(seed, mult):
    sd = weights.init_state_dict(seed)
    return F.scaled(sd, mult) if mult != 1 else sd


def _refs(seed, mult):
    """(emu64, emu32, fp64 torch) of the test boards, computed once per weight set."""
    if (seed, mult) not in _REF:
        planes = boards.planes_from_cells(_cells())
        sd = _sd(seed, mult)
        _REF[seed, mult] = (F.emulate(sd, planes, torch.float64), F.emulate(sd, planes, torch.float32),
                            F.torch_fp64(sd, planes))
    return _REF[seed, mult]


def _weights(seed, mult, prec):
    if (seed, mult, prec) not in _W:
        _W[seed, mult, prec] = device.PVWeights(weights.pack_pv_weights(_sd(seed, mult)), precision=prec)
    return _W[seed, mult, prec]


def _gpu(seed, mult, prec):
    """(logits, value, softmax) of all the test boards in one call (n = CUs + 3)."""
    if (seed, mult, prec) not in _GPU:
        _GPU[seed, mult, prec] = device.pv_forward(_weights(seed, mult, prec), _rows(_cells()))
    return _GPU[seed, mult, prec]


@pytest.mark.parametrize("seed,mult", [(0, 1), (1, 1), (0, 3), (1, 3)])
def test_f16_accuracy_against_the_cpu_restatement(seed, mult):
    e64, e32, t64 = _refs(seed, mult)
    g = _gpu(seed, mult, "f16")
    x3 = _gpu(seed, mult, "f16x3")
    fails = []
    for i, name in enumerate(("logits", "value", "softmax")):
        E = np.abs(e64[i] - t64[i]).max()
        D = np.abs(e32[i] - e64[i]).max()
        ge = np.abs(g[i].astype(np.float64) - e64[i]).max()
        gt = np.abs(g[i].astype(np.float64) - t64[i]).max()
        gx = np.abs(g[i].astype(np.float64) - x3[i]).max()
        print(f"seed {seed} x{mult} {name}: E {E:.3e} D {D:.3e} | gpu-emu64 {ge:.3e} ({ge / D:.2f} D) "
              f"gpu-fp64 {gt:.3e} gpu_f16-gpu_f16x3 {gx:.3e}")
        assert D > 0  # (the two CPU evaluations do differ: the bound is not empty)
        if not ge <= 4 * D:
            fails.append((name, "gpu - emu64", ge, 4 * D))
        if not gt <= E + 4 * D:
            fails.append((name, "gpu - fp64", gt, E + 4 * D))
        if i == 0 and not gx >= E / 4:
            fails.append((name, "f16 - f16x3", gx, E / 4))
    assert not fails, fails


@pytest.mark.parametrize("n", [1, 7])
def test_f16_small_batches_equal_the_large_one(n):
    """n = 1 and n = 7: the same bytes as the same boards' rows of the n = CUs + 3 call."""
    lg, v, pr = _gpu(0, 1, "f16")
    pick = np.array([5, 0, 2, _n_boards() - 1, 100, 4, 77][:n])
    got = device.pv_forward(_weights(0, 1, "f16"), _rows(_cells()[pick]))
    assert np.array_equal(got[0], lg[pick]) and np.array_equal(got[1], v[pick]) and np.array_equal(got[2], pr[pick])


def test_f16_second_board_of_a_workgroup():
    """n = CUs + 3: the last 3 boards are a workgroup's second board.  Evaluated alone (each
    the first board of its workgroup) they give the same bytes -- nothing of the first
    board is left in the LDS (zero slots intact, no lo plane to go stale)."""
    n = _n_boards()
    lg, v, pr = _gpu(0, 1, "f16")
    tail = np.arange(n - 3, n)
    got = device.pv_forward(_weights(0, 1, "f16"), _rows(_cells()[tail]))
    assert np.array_equal(got[0], lg[tail]) and np.array_equal(got[1], v[tail]) and np.array_equal(got[2], pr[tail])


def test_f16_device_count_below_n():
    """d_count = 10 of n = 64: rows 0..9 as in the full call, rows past the count untouched."""
    w = _weights(0, 1, "f16")
    lg, v, pr = _gpu(0, 1, "f16")
    d_b = torch.from_numpy(_rows(_cells()[:64]).view(np.int32).copy()).cuda()
    d_cnt = torch.tensor([10], dtype=torch.int32, device="cuda")
    d_lg = torch.full((64 * 225,), 7.0, device="cuda")
    d_v = torch.full((64,), 7.0, device="cuda")
    d_p = torch.full((64 * 225,), 7.0, device="cuda")
    d_prior = torch.full((64 * 225,), 7.0, dtype=torch.float64, device="cuda")
    device.pv_forward_dev(w, d_b, 64, d_count=d_cnt, d_logits=d_lg, d_value=d_v, d_probs=d_p, d_prior=d_prior)
    torch.cuda.synchronize()
    glg, gv, gp = d_lg.cpu().numpy().reshape(64, 225), d_v.cpu().numpy(), d_p.cpu().numpy().reshape(64, 225)
    assert np.array_equal(glg[:10], lg[:10]) and np.array_equal(gv[:10], v[:10]) and np.array_equal(gp[:10], pr[:10])
    assert np.all(glg[10:] == 7.0) and np.all(gv[10:] == 7.0) and np.all(gp[10:] == 7.0)
    assert np.all(d_prior.cpu().numpy().reshape(64, 225)[10:] == 7.0)


def test_f16_batch_invariance():
    """5 boards alone, inside n = 70 at other rows among other boards, and at n = 1 each:
    equal with ==."""
    w = _weights(1, 3, "f16")
    cells = _cells()
    five = np.array([5, 9, 33, 120, 200])
    alone = device.pv_forward(w, _rows(cells[five]))
    at = np.array([69, 3, 41, 0, 17])
    batch = cells[np.arange(70) + 130].copy()
    batch[at] = cells[five]
    inside = device.pv_forward(w, _rows(batch))
    for k in range(3):
        assert np.array_equal(inside[k][at], alone[k]), k
    for j, b in enumerate(five):
        one = device.pv_forward(w, _rows(cells[b:b + 1]))
        for k in range(3):
            assert np.array_equal(one[k][0], alone[k][j]), (j, k)


def test_f16x3_is_unchanged_by_an_f16_call_on_the_same_workspace():
    """gz_pv_forward(F16X3) on 64 boards before and after a GZ_PV_F16 call with the same
    weights and workspace: byte-identical (no state leaks through the records or the
    heads' fragments), and the F16 call in between gives the F16 outputs."""
    w = device.PVWeights(weights.pack_pv_weights(_sd(0, 1)), precision="f16x3")
    rows = _rows(_cells()[:64])
    before = device.pv_forward(w, rows)
    ws = w.workspace.data_ptr()
    w.mode = _lib.GZ_PV_F16
    mid = device.pv_forward(w, rows)
    w.mode = _lib.GZ_PV_F16X3
    after = device.pv_forward(w, rows)
    assert w.workspace.data_ptr() == ws
    for k in range(3):
        assert before[k].tobytes() == after[k].tobytes(), k
        assert np.array_equal(mid[k], _gpu(0, 1, "f16")[k][:64]), k
    assert not np.array_equal(mid[0], before[0])


def test_precision_3_is_still_an_argument_error():
    w = _weights(0, 1, "f16")
    L = _lib.load()
    d_b = torch.zeros(16, dtype=torch.int32, device="cuda")
    d_lg = torch.full((225,), 7.0, device="cuda")
    d_v = torch.full((1,), 7.0, device="cuda")
    rc = L.gz_pv_forward(device.ptr(w.tensor), device.ptr(d_b), 1, None, device.ptr(d_lg), device.ptr(d_v), None, None,
                         device.ptr(w.workspace_for(1)), 3, device.stream())
    assert rc == -1 and b"precision" in L.gz_last_error()  # GZ_ERR_ARG
    torch.cuda.synchronize()
    assert float(d_v[0]) == 7.0 and bool((d_lg == 7.0).all())
