"""CPU restatement of the GZ_PV_F16X3 forward in torch, and the weight blob's
fp16 fragments taken apart and put back -- a helper of test_pv_f16x3_cpu.py /
test_gpu_pv_f16x3.py, not a test.

emulate(sd, planes, dtype, terms, drop): the specification evaluated in ``dtype``
  * conv0 on the 0/1 planes with w_hi + w_lo, the fp32 BN affine of weights._affine, ReLU;
  * each residual conv as conv(a_hi, w_hi) + conv(a_hi, w_lo) + conv(a_lo, w_hi) -- no
    a_lo * w_lo -- with a_hi = fp16(y), a_lo = fp16(y - a_hi) of the previous epilogue's
    output y = relu(acc * S + T (+ skip)), the skip the block input as stored (a_hi + a_lo);
    w_hi = fp16(w), w_lo = fp16(w - w_hi) unless ``terms`` gives the four pairs;
  * x2 feeds the heads unsplit; the heads (1x1 convs, policy_fc, value_fc1 / fc2, tanh,
    softmax) in ``dtype``.
float64 has exact products and (to ~1e-16) exact sums: the specification itself.  There
conv(a_hi, w_hi) + conv(a_hi, w_lo) is taken as conv(a_hi, w_hi + w_lo): the sum of two
fp16 values is exact in float64 and so is every product, the results differ by float64's
own rounding.

Blob helpers (weights.F16_RES0 / F16_STRIDE; a residual layer's segment is frag(hi) then
frag(lo), pack_pv_weights): fragments / with_fragments, and on them swap_hi_lo and
truncate_lo.  conv0's fragments are left alone: its inputs are 0/1 and it sums the halves."""
import numpy as np
import torch
import torch.nn.functional as F

from gzero import weights

from pv_f16_ref import board_cells, scaled, torch_fp64  # noqa: F401  (re-exported)

CH, K = weights.CH, weights.K
_LAYERS = [(f"residual_tower.{i}.conv{c}", f"residual_tower.{i}.bn{c}") for i in range(2) for c in (1, 2)]


def weight_terms(sd):
    """The four residual layers' (w_hi, w_lo) as the packer cuts them, float64 [out][in][3][3]."""
    out = []
    for cn, bn in _LAYERS:
        w = weights._affine({k: v.detach().cpu() for k, v in sd.items()}, cn, bn)[0].float()
        hi = w.half()
        out.append((hi.double(), (w - hi.float()).half().double()))
    return out


def exact_terms(sd):
    """(fp16(w), w - fp16(w)) with the remainder unrounded: hi + lo == w."""
    out = []
    for cn, bn in _LAYERS:
        w = weights._affine({k: v.detach().cpu() for k, v in sd.items()}, cn, bn)[0].float().double()
        hi = w.half().double()
        out.append((hi, w - hi))
    return out


def emulate(sd, planes, dtype=torch.float64, terms=None, drop=(), exact=False):
    """planes [n,3,15,15] 0/1 -> (logits [n,225], value [n], softmax [n,225]) numpy ``dtype``.
    terms: four (w_hi, w_lo) in torch's conv layout instead of the split of sd's weights.
    drop: "w_lo" leaves conv(a_hi, w_lo) out, "a_lo" leaves conv(a_lo, w_hi) out.
    exact: every rounding of the specification off -- conv0 with w itself, S and T left in
    float64, a_lo = y - a_hi unrounded and the a_lo * w_lo product added (with
    terms = exact_terms(sd) this is the plain network)."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    if not set(drop) <= {"w_lo", "a_lo"}:
        raise ValueError(f"drop names w_lo and / or a_lo, not {drop!r}")
    x = torch.as_tensor(np.asarray(planes), dtype=dtype)
    if terms is None:
        terms = weight_terms(sd)

    def bn(cn, b):  # (S, T): the blob's fp32 pair; exact: the same fold left in float64
        if not exact:
            return weights._affine(sd, cn, b)[1:]
        g, beta, mean, var = (sd[f"{b}.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var"))
        s = g / torch.sqrt(var + weights.BN_EPS)
        return s, (sd[cn + ".bias"].double() - mean) * s + beta

    def affine(acc, s, t, skip=None):
        y = acc * s.to(dtype).view(1, -1, 1, 1) + t.to(dtype).view(1, -1, 1, 1)
        if skip is not None:
            y = y + skip
        return torch.relu(y)

    def split(y):
        hi = y.half().to(dtype)
        lo = y - hi
        return hi, (lo if exact else lo.half().to(dtype))

    def conv3(a, wt):
        (ah, al), (wh, wl) = a, (wt[0].to(dtype), wt[1].to(dtype))
        merged = dtype == torch.float64 and not drop
        acc = F.conv2d(ah, wh + wl if merged else wh, padding=1)
        if not merged and "w_lo" not in drop:
            acc = acc + F.conv2d(ah, wl, padding=1)
        if "a_lo" not in drop:
            acc = acc + F.conv2d(al, wh, padding=1)
        if exact:
            acc = acc + F.conv2d(al, wl, padding=1)
        return acc

    with torch.no_grad():
        w = sd["conv.weight"].float()
        s, t = bn("conv", "bn")
        if not exact:  # the two fp16 terms conv0 multiplies
            hi = w.half().float()
            w = hi.double() + (w - hi).half().double()
        h = split(affine(F.conv2d(x, w.to(dtype), padding=1), s, t))
        for i in range(2):
            (s1, t1), (s2, t2) = (bn(cn, b) for cn, b in _LAYERS[2 * i:2 * i + 2])
            y = split(affine(conv3(h, terms[2 * i]), s1, t1))
            out = affine(conv3(y, terms[2 * i + 1]), s2, t2, skip=h[0] + h[1])
            h = split(out)
        h = out  # x2 feeds the heads as the epilogue computed it
        return _heads(sd, out, dtype)  # x2 feeds the heads as the epilogue computed it


def _heads(sd, h, dtype):
    p = F.conv2d(h, sd["policy_conv.weight"].to(dtype), sd["policy_conv.bias"].to(dtype))
    lg = F.linear(torch.flatten(p, 1), sd["policy_fc.weight"].to(dtype), sd["policy_fc.bias"].to(dtype))
    v = F.conv2d(h, sd["value_conv.weight"].to(dtype), sd["value_conv.bias"].to(dtype))
    v = torch.relu(F.linear(torch.flatten(v, 1), sd["value_fc1.weight"].to(dtype), sd["value_fc1.bias"].to(dtype)))
    v = torch.tanh(F.linear(v, sd["value_fc2.weight"].to(dtype), sd["value_fc2.bias"].to(dtype)))
    return lg.numpy(), v.numpy().reshape(-1), torch.softmax(lg, dim=1).numpy()


def emulate_tree(sd, planes, meta, dtype=torch.float32, terms=None, drop=()):
    """The tree forward's arithmetic (csrc/gz_pvdg.hip's header comment) on whole boards:
    roots by the specification; a node tagged with its parent (a root, or a root's child)
    as a delta of it,
        z_node = z_parent + S * conv3(D) (+ D_skip),   D_next = relu(z_node) - relu(z_parent),
    z the pre-ReLU maps kept in ``dtype``, D split into fp16 hi / lo and multiplied by the
    same three terms; conv0 is evaluated on the node's own planes, D(x0) = x0 - x0_parent;
    the heads on relu(z) of the last layer.  Outside a node's changed square D is exactly 0,
    so whole boards give what the kernel's squares give.  In float32 this is a correct
    evaluation of the tree forward with another summation order: its distance from
    emulate(float64) is what the delta form itself costs (same returns as emulate).
    drop ("w_lo" / "a_lo") leaves that product out of the delta convolutions only -- the
    roots stay whole: a fault confined to pv_dg_kernel, for the CPU sensitivity test."""
    if not set(drop) <= {"w_lo", "a_lo"}:
        raise ValueError(f"drop names w_lo and / or a_lo, not {drop!r}")
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    meta = np.asarray(meta)
    x = torch.as_tensor(np.asarray(planes), dtype=dtype)
    terms = [(h.to(dtype), l.to(dtype)) for h, l in (weight_terms(sd) if terms is None else terms)]
    n = len(meta)

    def split(y):
        hi = y.half().to(dtype)
        return hi, (y - hi).half().to(dtype)

    def conv3(a, wt, drop=()):
        acc = F.conv2d(a[0], wt[0], padding=1)
        if "w_lo" not in drop:
            acc = acc + F.conv2d(a[0], wt[1], padding=1)
        if "a_lo" not in drop:
            acc = acc + F.conv2d(a[1], wt[0], padding=1)
        return acc

    def col(v):
        return v.to(dtype).view(1, -1, 1, 1)

    with torch.no_grad():
        w, s0, t0 = weights._affine(sd, "conv", "bn")
        w = w.float()
        hi = w.half().float()
        w0 = (hi.double() + (w - hi).half().double()).to(dtype)
        x0 = torch.relu(F.conv2d(x, w0, padding=1) * col(s0) + col(t0))
        st = [weights._affine(sd, cn, b)[1:] for cn, b in _LAYERS]
        z = [torch.zeros(n, CH, 15, 15, dtype=dtype) for _ in range(4)]
        roots = np.flatnonzero(meta == -1)
        kids = np.flatnonzero((meta >= 0) & (meta[np.maximum(meta, 0)] == -1))
        grand = np.flatnonzero((meta >= 0) & ~np.isin(np.arange(n), kids))
        h = split(x0[roots])
        for L in range(4):  # the roots: the full forward, z kept
            acc = conv3(h, terms[L]) * col(st[L][0]) + col(st[L][1])
            if L & 1:
                acc = acc + skip
            else:
                skip = h[0] + h[1]
            z[L][roots] = acc
            h = split(torch.relu(acc))
        for idx in (kids, grand):
            par = meta[idx]
            d = split(x0[idx] - x0[par])
            for L in range(4):
                acc = z[L][par] + conv3(d, terms[L], drop) * col(st[L][0])
                if L & 1:
                    acc = acc + skip
                else:
                    skip = d[0] + d[1]
                z[L][idx] = acc
                d = split(torch.relu(acc) - torch.relu(z[L][par]))
        return _heads(sd, torch.relu(z[3]), dtype)


def torch_fp32(sd, planes):
    """weights.reference_forward (torch fp32 on the CPU) with its softmax: (logits, value, softmax)."""
    lg, v = weights.reference_forward(sd, np.asarray(planes))
    return lg, v, torch.softmax(torch.from_numpy(lg), dim=1).numpy()


# ---------------------------------------------------------------- the blob's fp16 fragments
def _seg(blob, j):
    fb = weights.F16_RES0 + j * weights.F16_STRIDE
    return blob[fb:fb + weights.F16_STRIDE].view(np.float16)  # 2 K CH halves: frag(hi), frag(lo)


def _unfrag(a):  # [ks 36][nt 8][q 4][li 16][j 8] -> [out][in][3][3]
    wt = a.reshape(36, 8, 4, 16, 8).transpose(1, 3, 0, 2, 4).reshape(CH, 3, 3, CH)  # [n][kh][kw][cin]
    return np.ascontiguousarray(wt.transpose(0, 3, 1, 2))


def _frag(w):  # [out][in][3][3] -> the packer's frag of W^T [n][k], k = (kh*3+kw)*128 + cin
    wt = np.asarray(w, np.float16).transpose(0, 2, 3, 1).reshape(CH, K)
    return wt.reshape(8, 16, 36, 4, 8).transpose(2, 0, 3, 1, 4).reshape(-1)


def fragments(blob, j):
    """Residual layer j's (hi, lo) as fp16 [out][in][3][3]: the inverse of pack_pv_weights' frag."""
    h = _seg(np.ascontiguousarray(blob, np.float32), j)
    return _unfrag(h[:K * CH]), _unfrag(h[K * CH:])


def with_fragments(blob, j, hi, lo):
    """A copy of blob with residual layer j's fragments replaced by (hi, lo)."""
    out = np.array(blob, np.float32, copy=True)
    _seg(out, j)[:] = np.concatenate([_frag(hi), _frag(lo)])
    return out


def blob_terms(blob):
    """The four (hi, lo) of a blob as float64 tensors: emulate's ``terms``."""
    return [tuple(torch.from_numpy(x.astype(np.float64)) for x in fragments(blob, j)) for j in range(4)]


def swap_hi_lo(blob):
    """Every residual layer's hi and lo fragments exchanged: the lo path carries fp16(w)."""
    for j in range(4):
        hi, lo = fragments(blob, j)
        blob = with_fragments(blob, j, lo, hi)
    return blob


def truncate_lo(blob, bits):
    """Every residual layer's lo fragment cut to ``bits`` of fp16's 10 mantissa bits (towards zero)."""
    mask = np.uint16(0xFFFF & ~((1 << (10 - bits)) - 1))
    for j in range(4):
        hi, lo = fragments(blob, j)
        blob = with_fragments(blob, j, hi, (lo.view(np.uint16) & mask).view(np.float16))
    return blob


# ---------------------------------------------------------------- weight sets and the bound
SETS = [(0, 1), (1, 1), (0, 3), (1, 3), (0, 0.1)]  # (init seed, conv-weight multiplier); 0.1: w_lo subnormal
NAMES = ("logits", "value", "softmax")


def state(seed, mult):
    sd = weights.init_state_dict(seed)
    return scaled(sd, mult) if mult != 1 else sd


def fp32_error(sd, planes):
    """(fp64 net, T): T[i] = max |torch fp32 on the CPU - fp64 net| of logits, value, softmax on
    these boards and weights -- what fp32 itself costs here.  BOUND = 8 T: 4 for ~22-bit
    operands against fp32's 24, times 2 for another summation order (tests/gnet_cases.py)."""
    t64 = torch_fp64(sd, planes)
    t32 = torch_fp32(sd, planes)
    return t64, [float(np.abs(t32[i] - t64[i]).max()) for i in range(3)]


def dist(a, b):
    """max |a - b| per output of two (logits, value, softmax) triples, in float64."""
    return [float(np.abs(np.asarray(a[i], np.float64) - np.asarray(b[i], np.float64)).max()) for i in range(3)]
