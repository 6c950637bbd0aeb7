"""Planner-net test cases that carry signal: weights, boards, float64 references
and the tolerances derived from them (shared by test_gnet_signal_cpu.py,
test_gpu_gnet.py and tests/golden/make_golden.py).

GraphNet has no normalisation, so at the plain +-1/sqrt(fan_in) initialisation
nine conv + ReLU layers shrink the board-dependent part of the activations to
~3e-5 of a logit: the biases alone decide the outputs and a wrong tower passes
any absolute tolerance.  Here the embed and the eight layer conv weights are
multiplied by GAIN, which keeps every layer's largest activation of order 1
(test_gnet_signal_cpu.py asserts the range), so a wrong layer reaches the logits.

Every tolerance comes from the references alone: FACTOR x the largest error of
torch's fp32 CPU forward against the float64 forward on the same boards and
weights.  FACTOR = 8 = 4 x 2: the f16x3 operands (hi + lo fp16) carry ~22 bits
against fp32's 24, and the kernels sum in another order.  q takes the same factor:
the fp32-MFMA heads (fc0 restated as base + stone deltas, K = 675) measured 1.5e-7 /
1.3e-7 against float64 on an MI355X where TOL_Q was 5.6e-7 / 6.5e-7 (cases 0 / 1), so
no summation-length allowance is needed.  Logits: 1.7e-6 / 1.1e-6 against 4.7e-6 /
4.2e-6; p: 1.9e-8 / 7.6e-9 against 4.0e-8 / 3.5e-8 (DESIGN 3.4b has the kept maps).
"""
import base64
import functools

import numpy as np
import torch
import torch.nn.functional as F

from gzero import boards, planner_nets

GAIN = 2.5
# (GraphNet seed, OpponentDQN seed): the fixtures' pair and a second one
CASES = ((21, 22), (4, 9))
N_BOARDS = 96
SIZES = (1, 33, 96)  # launch sizes: across the 16- and 32-board workgroup edges
FACTOR = 8
ACT_RANGE = (0.5, 8.0)  # per-layer max activation of the float64 reference
LAYERS = ["embed"] + [f"layers.{i}" for i in range(8)]
SLOT_MAPS = (0, 2, 4, 6)  # the kept maps (embed, L1, L3, L5) as indices into LAYERS
GOLDEN_CASE, GOLDEN_BOARDS = 1, tuple(range(0, N_BOARDS, 3))  # gnet2.json.gz: 32 boards of case 1


def graphnet_state(seed, gain=GAIN):
    """init_graphnet_state(seed) with the embed and layer conv weights x gain
    (biases and the policy head as initialised)."""
    sd = planner_nets.init_graphnet_state(seed)
    for name in LAYERS:
        sd[name + ".weight"] = sd[name + ".weight"] * np.float32(gain)
    return sd


def dqn_state(seed):
    return planner_nets.init_dqn_state(seed)


@functools.lru_cache(None)
def board_cells():
    """[96, 225] int8 cells (0 empty / 1 black / 2 white): the empty and the full board,
    single stones in the corners, on an edge and in the centre, one-colour boards,
    random boards at three densities.  Board 0 is the empty board (the n = 1 launch)."""
    rng = np.random.default_rng(77)
    out = [np.zeros(225, np.int8), rng.choice([1, 2], size=225).astype(np.int8)]
    for colour in (1, 2):
        for cell in (0, 14, 112, 210, 224):
            c = np.zeros(225, np.int8)
            c[cell] = colour
            out.append(c)
    for colour in (1, 2):  # one colour only: full, then sparse to dense
        out.append(np.full(225, colour, np.int8))
        for dens in (0.05, 0.3, 0.7):
            out.append((colour * (rng.random(225) < dens)).astype(np.int8))
    dens = (0.1, 0.5, 0.9)
    k = 0
    while len(out) < N_BOARDS:
        d = dens[k % 3]
        out.append(rng.choice(3, size=225, p=[1 - d, d / 2, d / 2]).astype(np.int8))
        k += 1
    cells = np.stack(out)
    cells.setflags(write=False)
    return cells


def encode_f32(a):
    return base64.b64encode(np.ascontiguousarray(a, np.float32).tobytes()).decode()


def decode_f32(s, shape):
    return np.frombuffer(base64.b64decode(s), dtype=np.float32).reshape(shape)


def planes_of(cells, dtype=torch.float64):
    return torch.from_numpy(boards.planes_from_cells(cells)).to(dtype)


def gn_forward(gsd, planes, dtype=torch.float64):
    """GraphNet in `dtype` on the CPU -> (activations of the nine conv + ReLU layers
    [n, 64, 225] each, policy-conv output [n, 450] channel-major, logits, p)."""
    w = {k: v.to(dtype) for k, v in gsd.items()}
    x = planes.to(dtype)
    acts = []
    with torch.no_grad():
        h = F.relu(F.conv2d(x, w["embed.weight"], w["embed.bias"], padding=1))
        acts.append(h)
        for i in range(8):
            h = F.relu(F.conv2d(h, w[f"layers.{i}.weight"], w[f"layers.{i}.bias"], padding=1 - i % 2))
            acts.append(h)
        pol = F.conv2d(h, w["policy_head.0.weight"], w["policy_head.0.bias"]).flatten(1)
        logits = F.linear(pol, w["policy_head.2.weight"], w["policy_head.2.bias"])
        p = torch.softmax(logits, dim=1)
    return [a.flatten(2).numpy() for a in acts], pol.numpy(), logits.numpy(), p.numpy()


def dqn_forward(dsd, planes, dtype=torch.float64):
    w = {k: v.to(dtype) for k, v in dsd.items()}
    with torch.no_grad():
        h = planes.to(dtype).flatten(1)
        h = F.relu(F.linear(h, w["net.0.weight"], w["net.0.bias"]))
        h = F.relu(F.linear(h, w["net.2.weight"], w["net.2.bias"]))
        return F.linear(h, w["net.4.weight"], w["net.4.bias"]).numpy()


class Case:
    """One weight set on the board set: the state dicts, the float64 reference and the
    tolerances (FACTOR x the fp32 forward's error against it)."""

    def __init__(self, idx):
        self.idx = idx
        self.gn_seed, self.dqn_seed = CASES[idx]
        self.gsd, self.dsd = graphnet_state(self.gn_seed), dqn_state(self.dqn_seed)
        self.cells = board_cells()
        x = planes_of(self.cells)
        self.acts, self.pol, self.logits, self.p = gn_forward(self.gsd, x)
        self.q = dqn_forward(self.dsd, x)
        a32, pol32, lg32, p32 = gn_forward(self.gsd, x, torch.float32)
        q32 = dqn_forward(self.dsd, x, torch.float32)
        err = lambda a, b: float(np.abs(a.astype(np.float64) - b).max())
        self.e32_lg, self.e32_p, self.e32_q = err(lg32, self.logits), err(p32, self.p), err(q32, self.q)
        self.e32_act = [err(a, b) for a, b in zip(a32, self.acts)]
        self.e32_pol = err(pol32, self.pol)
        self.tol_lg, self.tol_p, self.tol_q = FACTOR * self.e32_lg, FACTOR * self.e32_p, FACTOR * self.e32_q
        self.tol_act = [FACTOR * e for e in self.e32_act]
        self.tol_pol = FACTOR * self.e32_pol

    def blob(self):
        return planner_nets.pack_planner_weights(self.gsd, self.dsd)

    def rows(self, n=N_BOARDS):
        bl, wh = boards.cells_to_words(self.cells[:n])
        return boards.leaf_words(bl, wh)


@functools.lru_cache(None)
def case(idx):
    return Case(idx)
