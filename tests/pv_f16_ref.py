"""CPU restatement of the GZ_PV_F16 forward (include/gzero.h) in torch -- a helper of
test_pv_f16_cpu.py / test_gpu_pv_f16.py, not a test.

emulate(sd, planes, dtype): the specification evaluated in ``dtype``
  * conv0 on the 0/1 planes with w_hi + w_lo (fp16(w) + fp16(w - fp16(w))), the fp32 BN
    affine of weights._affine, ReLU; x0 rounded to fp16;
  * each residual conv with fp16(w) on the stored fp16 map, y = relu(acc * S + T (+ skip)),
    skip the block input as stored; y1, x1, y2 rounded to fp16, x2 not;
  * the heads (1x1 convs, policy_fc, value_fc1 / fc2, tanh, softmax) in ``dtype``.
float64 has exact products and (to ~1e-16) exact sums: the specification itself.
float32 is the same specification with another accumulation rounding, like the kernel's;
the two differ where an accumulation error moves a value across an fp16 rounding
boundary.  rounding=False switches every fp16 rounding off (the plain network, to be
compared with weights.reference_forward)."""
import numpy as np
import torch
import torch.nn.functional as F

from gzero import weights


def _r16(x, on):
    return x.half().to(x.dtype) if on else x


def emulate(sd, planes, dtype=torch.float64, rounding=True):
    """planes [n,3,15,15] 0/1 -> (logits [n,225], value [n], softmax [n,225]) numpy ``dtype``."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    x = torch.as_tensor(np.asarray(planes), dtype=dtype)

    def affine(y, s, t, skip=None):
        y = y * s.to(dtype).view(1, -1, 1, 1) + t.to(dtype).view(1, -1, 1, 1)
        if skip is not None:
            y = y + skip
        return torch.relu(y)

    with torch.no_grad():
        w, s, t = weights._affine(sd, "conv", "bn")
        w = w.float()
        if rounding:  # the two fp16 terms conv0 multiplies
            hi = w.half().float()
            w = (hi.double() + (w - hi).half().double())
        h = _r16(affine(F.conv2d(x, w.to(dtype), padding=1), s, t), rounding)
        for i in range(2):
            w1, s1, t1 = weights._affine(sd, f"residual_tower.{i}.conv1", f"residual_tower.{i}.bn1")
            w2, s2, t2 = weights._affine(sd, f"residual_tower.{i}.conv2", f"residual_tower.{i}.bn2")
            w1, w2 = (_r16(a.float(), rounding).to(dtype) for a in (w1, w2))
            y = _r16(affine(F.conv2d(h, w1, padding=1), s1, t1), rounding)
            h = affine(F.conv2d(y, w2, padding=1), s2, t2, skip=h)
            if i == 0:
                h = _r16(h, rounding)  # x1 is stored; x2 feeds the heads unrounded
        p = F.conv2d(h, sd["policy_conv.weight"].to(dtype), sd["policy_conv.bias"].to(dtype))
        lg = F.linear(torch.flatten(p, 1), sd["policy_fc.weight"].to(dtype), sd["policy_fc.bias"].to(dtype))
        v = F.conv2d(h, sd["value_conv.weight"].to(dtype), sd["value_conv.bias"].to(dtype))
        v = torch.relu(F.linear(torch.flatten(v, 1), sd["value_fc1.weight"].to(dtype), sd["value_fc1.bias"].to(dtype)))
        v = torch.tanh(F.linear(v, sd["value_fc2.weight"].to(dtype), sd["value_fc2.bias"].to(dtype)))
        return lg.numpy(), v.numpy().reshape(-1), torch.softmax(lg, dim=1).numpy()


def torch_fp64(sd, planes):
    """The network itself (no fp16 anywhere) in float64: (logits, value, softmax)."""
    net = weights.PolicyValueNet().double()
    net.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
    net.eval()
    with torch.no_grad():
        lg, v = net(torch.as_tensor(np.asarray(planes), dtype=torch.float64))
    return lg.numpy(), v.numpy().reshape(-1), torch.softmax(lg, dim=1).numpy()


def scaled(sd, mult):
    """sd with every 4-D (conv) weight times mult."""
    return {k: (v * mult if v.dim() == 4 else v) for k, v in sd.items()}


def board_cells(n, seed=0):
    """n boards [n,225] int8: empty, one stone in each corner, a 120-stone board, the
    rest random with 0..119 stones (colours alternating as in play)."""
    rng = np.random.default_rng(seed)
    cells = np.zeros((n, 225), np.int8)
    for i, c in enumerate((0, 14, 210, 224)):
        cells[1 + i, c] = 1 + i % 2
    for i in range(5, n):
        k = 120 if i == 5 else int(rng.integers(0, 120))
        at = rng.permutation(225)[:k]
        cells[i, at[0::2]] = 1
        cells[i, at[1::2]] = 2
    return cells
