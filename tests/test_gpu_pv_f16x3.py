"""The f16x3 forwards on the GPU held to their claim: fp32-equivalent products,
not "within 1e-4".

Reference and bound (tests/pv_f16x3_ref.py; the conditions that give them their meaning
are asserted without a GPU in tests/test_pv_f16x3_cpu.py):
    emu64 = the three-term specification a_hi w_hi + a_hi w_lo + a_lo w_hi evaluated in
            float64, with the (w_hi, w_lo) fragments the blob under test holds;
    T     = max |torch fp32 on the CPU - float64 network| on the same boards and weights,
            per output (logits, value, softmax): what fp32 itself costs there;
    BOUND = 8 T: 4 for ~22-bit operands against fp32's 24, times 2 for another summation
            order (the project's number for this arithmetic, tests/gnet_cases.py).
Nothing here comes from a kernel's output.  Every comparison prints its error as a
multiple of its bound.

Full forward (gz_pv_forward), n = CUs + 3 boards of pv_f16_ref.board_cells, so that a
workgroup runs a second board; weight sets init seed 0 / 1 plain and conv weights x 3, and
seed 0 x 0.1 (w_lo subnormal):
  * pv_kernel_f16x3 within BOUND of emu64 -- with the CPU module's 4 T between emu64 and
    the network, within 12 T of the float64 network;
  * pv_kernel_f32 within BOUND of the float64 network;
  * the blob with every residual layer's hi and lo fragments exchanged (swap_hi_lo) against
    emu64 of the exchanged terms: wherever the kernel reads, holds or multiplies a lo weight
    fragment it now carries the whole weight, so a lost w_lo is an O(1) error (CPU module).
    BOUND does not hold here, for a correct evaluation either: with the a_lo path carrying
    only a_lo w_lo, an fp16 rounding of a map that the accumulation error flips is not made
    up for.  The specification accumulated in float32 on the CPU lies D = 6 to 43 BOUND from
    emu64 (MI355X run: the kernel 4 to 47 BOUND), so by the 4 D rule of test_gpu_pv_f16.py
    the bound is 4 D wherever D leaves BOUND.  A lost w_lo is still >= 1000 x that bound, one
    mantissa bit of ten shaved off it 1.6 to 1.8 x (CPU module's figures over 4 D);
  * negative control, no kernel change: the forward of truncate_lo(blob, 3) -- w_lo cut to 3
    mantissa bits, the 5 % faster variant DESIGN 3.3 declines -- against emu64 of the
    untouched weights is more than 8 BOUND away and less than 1e-4: the fault a 1e-4
    tolerance lets through, seen on the device.

Tree forward (gz_pv_forward_tree: pv_dg_kernel<false> for the root children,
pv_dg_kernel<true> for the grandchildren), sets (0, 1) and (1, 3), normal and exchanged
blobs.  A root of 4 stones with a child on every empty cell (every row class and clipped
square), grandchildren on every third empty cell under the parents at cells 0, 14, 112,
210, 224 (squares that overlap, clip and stay disjoint), a second root of 40 stones with
children on every fourth empty cell and grandchildren under two of them; the list counts
are asserted, so no row quietly took the full forward.
  * roots bitwise the full forward;
  * root children and grandchildren within 2 BOUND = 16 T of emu64 (same terms as the
    blob), T taken on these boards.  The 2 is derived: a delta row adds one more f32
    accumulation chain of at most the same length, and one more fp32 rounding of the
    stored z per layer, to what the full forward does.  With the exchanged blob the delta
    form of gz_pvdg.hip's header evaluated in float32 on the CPU (pv_f16x3_ref.emulate_tree:
    z in fp32, D = child - relu(z) split hi / lo) lies D = 6 to 45 x 2 BOUND from emu64 --
    fp16(parent) + fp16(D) is not fp16(child), and nothing makes it up when a_lo w_hi is
    gone -- and the kernel lands where it does (0.22 to 0.35 of 4 D); there the bound is
    4 D, per output and row group, wherever D leaves 2 BOUND.

What fails if a kernel loses w_lo, loses a_lo or shaves mantissa bits off either (ratios
from the CPU module and DESIGN 3.3's table):
  pv_kernel_f16x3      test_full_forward_f16x3 (either term, x 1 and x 3: >= 20 BOUND; w_lo cut
                       to 3 bits: 26 BOUND, the negative control) and test_full_forward_swapped
                       (w_lo lost: >= 1000 x its bound);
  pv_kernel_f32        test_full_forward_fp32 (any lost operand bits: the bound is 8 T);
  pv_dg_kernel<false>  test_tree_forward, children rows.  A term lost in the delta convolutions
                       alone, on these boards (pv_f16x3_ref.emulate_tree(drop=...), float64):
                       w_lo 1.5 x the bound at x 1 and 4.2 x at x 3, a_lo (the lo half of D)
                       1.6 x and 4.3 x, with the packer's blob; a library built without the
                       w_lo MFMA of the k-loop measured 1.53 x and 4.14 x on the MI355X, and
                       ~100 x with the exchanged blob;
  pv_dg_kernel<true>   test_tree_forward, grandchildren rows: w_lo 2.2 x and 6.7 x (the same
                       library: 2.15 x, 6.73 x, ~100 x exchanged), a_lo 2.2 x and 6.2 x.
"""
import numpy as np
import pytest
import torch

import pv_f16x3_ref as R
from gzero import boards, device, weights
from test_gpu_pvinc import _concat, _grand_family, _root_family

pytestmark = pytest.mark.gpu

_C = {}


def _rows(cells):
    bl, wh = boards.cells_to_words(np.asarray(cells, np.int8).reshape(-1, 225))
    return boards.leaf_words(bl, wh)


def _full_cells():
    if "cells" not in _C:
        n = torch.cuda.get_device_properties(0).multi_processor_count + 3  # 259 on the MI355X
        _C["cells"] = R.board_cells(n, seed=0)
    return _C["cells"]


def _refs(kind, cells_fn, seed, mult, blob_name="normal"):
    """CPU references of one weight set on one board list, computed once: the float64 network,
    T, and emu64 with the named blob's terms."""
    key = (kind, seed, mult)
    if key not in _C:
        sd = R.state(seed, mult)
        planes = boards.planes_from_cells(np.asarray(cells_fn(), np.int8).reshape(-1, 225))
        t64, T = R.fp32_error(sd, planes)
        blob = weights.pack_pv_weights(sd)
        _C[key] = dict(sd=sd, planes=planes, t64=t64, T=T, blobs={"normal": blob}, emu={})
    s = _C[key]
    if blob_name == "swapped" and "swapped" not in s["blobs"]:
        s["blobs"]["swapped"] = R.swap_hi_lo(s["blobs"]["normal"])
    if blob_name not in s["emu"]:
        s["emu"][blob_name] = R.emulate(s["sd"], s["planes"], terms=R.blob_terms(s["blobs"][blob_name]))
    return s


def _within(what, got, ref, T, factor=8, rows=None, cpu32=None):
    """Print max |got - ref| per output as a multiple of its bound; return the outputs past it.
    The bound is factor * T.  cpu32 (exchanged blobs only): a correct float32 evaluation of
    the same arithmetic on the CPU; where its own distance D from ref leaves factor * T, the
    bound is 4 D instead (the 4 D rule of test_gpu_pv_f16.py)."""
    fails = []
    for i, name in enumerate(R.NAMES):
        g, r = np.asarray(got[i], np.float64), np.asarray(ref[i], np.float64)
        if rows is not None:
            g, r = g[rows], r[rows]
        err, bound, rule = float(np.abs(g - r).max()), factor * T[i], f"{factor} T"
        if cpu32 is not None:
            c = np.asarray(cpu32[i], np.float64)
            D = float(np.abs((c if rows is None else c[rows]) - r).max())
            if D > bound:
                rule = f"4 D, D = {D / bound:.2f} x {factor} T"
                bound = 4 * D
        print(f"{what} {name}: {err:.3e} = {err / bound:.3f} x bound ({bound:.3e} = {rule})")
        if not err <= bound:
            fails.append((what, name, err, bound))
    return fails


@pytest.mark.parametrize("seed,mult", R.SETS)
def test_full_forward_f16x3(seed, mult):
    s = _refs("full", _full_cells, seed, mult)
    got = device.pv_forward(device.PVWeights(s["blobs"]["normal"], precision="f16x3"), _rows(_full_cells()))
    fails = _within(f"f16x3 seed {seed} x{mult} gpu - emu64", got, s["emu"]["normal"], s["T"])
    assert not fails, fails


@pytest.mark.parametrize("seed,mult", R.SETS)
def test_full_forward_fp32(seed, mult):
    s = _refs("full", _full_cells, seed, mult)
    got = device.pv_forward(device.PVWeights(s["blobs"]["normal"], precision="fp32"), _rows(_full_cells()))
    fails = _within(f"fp32 seed {seed} x{mult} gpu - fp64 net", got, s["t64"], s["T"])
    assert not fails, fails


@pytest.mark.parametrize("seed,mult", [(0, 1), (1, 3)])
def test_full_forward_swapped(seed, mult):
    s = _refs("full", _full_cells, seed, mult, "swapped")
    got = device.pv_forward(device.PVWeights(s["blobs"]["swapped"], precision="f16x3"), _rows(_full_cells()))
    cpu32 = R.emulate(s["sd"], s["planes"], torch.float32, terms=R.blob_terms(s["blobs"]["swapped"]))
    fails = _within(f"f16x3 swapped seed {seed} x{mult} gpu - emu64(swapped)", got, s["emu"]["swapped"], s["T"], cpu32=cpu32)
    assert not fails, fails


def test_truncated_w_lo_is_outside_the_bound_and_inside_1e_4():
    s = _refs("full", _full_cells, 0, 1)
    cut = R.truncate_lo(s["blobs"]["normal"], 3)
    got = device.pv_forward(device.PVWeights(cut, precision="f16x3"), _rows(_full_cells()))
    err = R.dist(got, s["emu"]["normal"])[0]
    bound = 8 * s["T"][0]
    print(f"w_lo cut to 3 bits, gpu - emu64 logits: {err:.3e} = {err / bound:.1f} x BOUND ({bound:.3e})")
    assert err > 8 * bound, (err, bound)
    assert err < 1e-4, err


# ---------------------------------------------------------------- tree forward
def _tree_boards():
    if "tree" not in _C:
        rng = np.random.default_rng(20251003)
        fam1 = _grand_family(rng, 4, [0, 14, 112, 210, 224], every=3)
        root, kids = _root_family(rng, 40)
        kids = kids[::4]
        cells, meta = [root] + kids, [-1] + [0] * len(kids)
        for p in (1, 1 + len(kids) // 2):  # a corner child and one in the middle
            for c in np.flatnonzero(cells[p] == 0)[::3]:
                g = cells[p].copy()
                g[c] = 2  # 40 stones: black moved, white answers
                cells.append(g)
                meta.append(p)
        _C["tree"] = _concat([fam1, (cells, meta)])
    return _C["tree"]


def _tree_cells():
    return _tree_boards()[0]


@pytest.mark.parametrize("blob_name", ["normal", "swapped"])
@pytest.mark.parametrize("seed,mult", [(0, 1), (1, 3)])
def test_tree_forward(seed, mult, blob_name):
    cells, meta = _tree_boards()
    m = np.asarray(meta)
    roots = np.flatnonzero(m == -1)
    kids = np.flatnonzero((m >= 0) & (m[np.maximum(m, 0)] == -1))
    grand = np.flatnonzero((m >= 0) & (m[np.maximum(m, 0)] >= 0))
    n_par = len(np.unique(m[grand]))
    assert len(roots) == 2 and len(kids) == 221 + 47 and n_par == 7 and len(grand) == 5 * 74 + 2 * 62
    s = _refs("tree", _tree_cells, seed, mult, blob_name)
    w = device.PVWeights(s["blobs"][blob_name], precision="f16x3")
    rows = _rows(cells)
    full = device.pv_forward(w, rows, want_prior=True)
    tree = device.pv_forward_tree(w, rows, meta)
    assert tree[4] == [2, 2, len(kids), 0, len(grand), n_par], tree[4]
    for k in range(4):
        assert np.array_equal(tree[k][roots], full[k][roots]), k
    ref = s["emu"][blob_name]
    what = f"tree {blob_name} seed {seed} x{mult}"
    cpu32 = None
    if blob_name == "swapped":
        cpu32 = R.emulate_tree(s["sd"], s["planes"], meta, torch.float32, terms=R.blob_terms(s["blobs"][blob_name]))
    fails = _within(f"{what} root children - emu64", tree, ref, s["T"], 16, kids, cpu32)
    fails += _within(f"{what} grandchildren - emu64", tree, ref, s["T"], 16, grand, cpu32)
    assert not fails, fails
