"""The planner-net cases of gnet_cases.py discriminate: on these boards and weights a
wrong GraphNet / OpponentDQN moves the float64 reference's outputs far above the
tolerances the GPU tests (test_gpu_gnet.py) hold the kernels to.  Conditions on the
inputs only -- nothing here runs a kernel.  If one falls short, change the boards or
the gain in gnet_cases.py, not the factors."""
import numpy as np
import pytest
import torch

import gnet_cases as gc
from conftest import golden
from gzero import planner_nets

SIGNAL_X = 100  # board-to-board std of an output >= SIGNAL_X x its tolerance
MUT_X = 10      # a mutated reference moves an output by >= MUT_X x its tolerance

CASE_IDS = list(range(len(gc.CASES)))


def _clone(sd):
    return {k: v.clone() for k, v in sd.items()}


def _busiest(act):
    """channel with the largest mean activation ([n, 64, 225]): a live one"""
    return int(act.mean(axis=(0, 2)).argmax())


def gn_mutations(c):
    """(name, state dict, planes) of every GraphNet mutation"""
    x = gc.planes_of(c.cells)
    out = []
    for i, name in enumerate(gc.LAYERS):  # the f16x3 lo term of one layer lost
        sd = _clone(c.gsd)
        sd[name + ".weight"] = sd[name + ".weight"].half().float()
        out.append((f"{name} weights -> fp16", sd, x))
    for i, name in enumerate(gc.LAYERS):  # a dropped bias (of a channel that is live)
        sd = _clone(c.gsd)
        sd[name + ".bias"][_busiest(c.acts[i])] = 0
        out.append((f"{name} one bias zeroed", sd, x))
    for i in (1, 3, 5, 7):  # 1x1 layers
        sd = _clone(c.gsd)
        sd[f"layers.{i}.weight"][_busiest(c.acts[i + 1])] = 0
        out.append((f"layers.{i} (1x1) one output channel zeroed", sd, x))
    for i, tap in ((0, (0, 0)), (2, (0, 2)), (4, (1, 1)), (6, (2, 0))):  # 3x3 layers
        sd = _clone(c.gsd)
        sd[f"layers.{i}.weight"][:, :, tap[0], tap[1]] = 0
        out.append((f"layers.{i} (3x3) tap {tap} zeroed", sd, x))
    for plane in range(3):  # an input plane misread on the edge ring of the board
        xe = x.clone().reshape(-1, 3, 15, 15)
        xe[:, plane, 0, :] = xe[:, plane, 14, :] = 0
        xe[:, plane, :, 0] = xe[:, plane, :, 14] = 0
        out.append((f"embed input plane {plane} zeroed on the edge ring", c.gsd, xe))
    sd = _clone(c.gsd)
    sd["policy_head.0.weight"] = sd["policy_head.0.weight"].flip(0)
    sd["policy_head.0.bias"] = sd["policy_head.0.bias"].flip(0)
    out.append(("policy-conv channels swapped", sd, x))
    sd = _clone(c.gsd)
    sd["policy_head.2.weight"][112] = 0
    out.append(("policy FC row 112 zeroed", sd, x))
    return out


def dqn_mutations(c):
    out = []
    sd = _clone(c.dsd)
    sd["net.0.weight"][:, 2 * 225 + 7] = 0  # the "empty" input of cell 7
    out.append(("fc0 column zeroed", sd))
    for k in (0, 2, 4):
        sd = _clone(c.dsd)
        sd[f"net.{k}.bias"][int(sd[f"net.{k}.bias"].abs().argmax())] = 0
        out.append((f"net.{k} one bias zeroed", sd))
    sd = _clone(c.dsd)
    sd["net.4.weight"][112] = 0
    out.append(("fc2 row 112 zeroed", sd))
    return out


@pytest.mark.parametrize("idx", CASE_IDS)
def test_activation_range(idx):
    c = gc.case(idx)
    mx = [float(a.max()) for a in c.acts]
    print(f"\ncase {idx} (GraphNet seed {c.gn_seed}, gain {gc.GAIN}) per-layer max activation: "
          + " ".join(f"{m:.2f}" for m in mx))
    assert all(gc.ACT_RANGE[0] <= m <= gc.ACT_RANGE[1] for m in mx), mx


@pytest.mark.parametrize("idx", CASE_IDS)
def test_tolerances_and_signal(idx):
    c = gc.case(idx)
    std_lg = float(c.logits.std(axis=0).mean())
    std_p = float(c.p.std(axis=0).mean())
    std_q = float(c.q.std(axis=0).mean())
    print(f"\ncase {idx}: fp32 vs float64 max error: logits {c.e32_lg:.2e}  p {c.e32_p:.2e}  q {c.e32_q:.2e}")
    print(f"  TOL_LG {c.tol_lg:.2e}  TOL_P {c.tol_p:.2e}  TOL_Q {c.tol_q:.2e}")
    print("  per-layer activation tolerance: " + " ".join(f"{t:.1e}" for t in c.tol_act) + f"  pol {c.tol_pol:.1e}")
    print(f"  board-to-board std: logits {std_lg:.2e} ({std_lg / c.tol_lg:.0f} x TOL_LG)  "
          f"p {std_p:.2e} ({std_p / c.tol_p:.0f} x TOL_P)  q {std_q:.2e} ({std_q / c.tol_q:.0f} x TOL_Q)")
    assert 0 < c.tol_lg < 1e-4 and 0 < c.tol_p < 1e-6 and 0 < c.tol_q < 1e-4  # tighter than the old absolute ones
    assert std_lg >= SIGNAL_X * c.tol_lg
    assert std_p >= SIGNAL_X * c.tol_p
    assert std_q >= SIGNAL_X * c.tol_q


@pytest.mark.parametrize("idx", CASE_IDS)
def test_graphnet_mutations_show(idx):
    c = gc.case(idx)
    rows, short = [], []
    for name, sd, x in gn_mutations(c):
        lg = gc.gn_forward(sd, x)[2]
        d = float(np.abs(lg - c.logits).max())
        rows.append(f"  {name:52s} max |dlogit| {d:.2e} = {d / c.tol_lg:8.0f} x TOL_LG")
        if d < MUT_X * c.tol_lg:
            short.append(name)
    print(f"\ncase {idx} (TOL_LG {c.tol_lg:.2e}):\n" + "\n".join(rows))
    assert not short, short


@pytest.mark.parametrize("idx", CASE_IDS)
def test_dqn_mutations_show(idx):
    c = gc.case(idx)
    x = gc.planes_of(c.cells)
    rows, short = [], []
    for name, sd in dqn_mutations(c):
        d = float(np.abs(gc.dqn_forward(sd, x) - c.q).max())
        rows.append(f"  {name:52s} max |dq| {d:.2e} = {d / c.tol_q:8.0f} x TOL_Q")
        if d < MUT_X * c.tol_q:
            short.append(name)
    print(f"\ncase {idx} (TOL_Q {c.tol_q:.2e}):\n" + "\n".join(rows))
    assert not short, short


def test_board_set():
    cells = gc.board_cells()
    assert cells.shape == (gc.N_BOARDS, 225) and len({c.tobytes() for c in cells}) == gc.N_BOARDS
    assert not cells[0].any() and (cells[1] != 0).all()
    stones = (cells != 0).sum(axis=1)
    for colour in (1, 2):
        for cell in (0, 14, 112, 210, 224):
            assert any(s == 1 and c[cell] == colour for s, c in zip(stones, cells))
        assert any((c == colour).all() for c in cells)


def test_reference_forward_reproduces_fixture():
    """gnet2.json.gz was written by the reference's own GraphNet / OpponentDQN (fp32 torch)
    at the signal gain; the project's restatement of the nets gives the same outputs.
    Both are fp32 forwards of the same nets, each within its fp32 error of float64."""
    g = golden("gnet2")
    c = gc.case(gc.GOLDEN_CASE)
    assert (g["gn_seed"], g["dqn_seed"], g["gain"]) == (c.gn_seed, c.dqn_seed, gc.GAIN)
    assert tuple(g["boards"]) == gc.GOLDEN_BOARDS
    cells = np.array([[int(ch) for ch in s] for s in g["cells"]], np.int8)
    assert np.array_equal(cells, c.cells[list(gc.GOLDEN_BOARDS)])
    n = len(cells)
    from gzero import boards
    lg, p, q = planner_nets.reference_forward(c.gsd, c.dsd, boards.planes_from_cells(cells))
    for name, got, e32 in (("logits", lg, c.e32_lg), ("p", p, c.e32_p), ("q", q, c.e32_q)):
        want = gc.decode_f32(g[name + "_f32_b64"], (n, 225))
        d = float(np.abs(got - want).max())
        print(f"{name}: max |restatement - reference| {d:.2e} (bound {2 * e32:.2e})")
        assert d <= 2 * e32
