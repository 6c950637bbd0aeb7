"""The PUCT search's leaf symmetry without a GPU: the transform of a position
(tests/puct_sym_ref.py against gz_pv_sym_host, the kernels' code on the host), the
reference's transform and map-back, the Python surface and the C argument errors."""
import ctypes

import numpy as np
import pytest

import puct_sym_ref as SR
from gzero import _lib, boards, device

SEEDS = (0, 3, 20240101)
ONE_STONE = [4, 3, 6, 7, 1, 3, 2, 7, 1, 1, 6, 0, 7, 6, 5, 2]  # seed 3, one black stone at cell 0..15


def _one_stone(c, colour=1):
    cells = [0] * 225
    cells[c] = colour
    return cells


def _rows4096():
    cells = np.random.RandomState(12345).randint(0, 3, (4096, 225))
    return np.array([SR.pack_row(c) for c in cells], np.uint32)


# ---------------------------------------------------------------- which transform
def test_known_answers():
    empty = [0] * 16
    assert SR.sym_of(3, empty) == 3 and SR.sym_of(0, empty) == 3
    assert [SR.sym_of(3, SR.pack_row(_one_stone(c))) for c in range(16)] == ONE_STONE
    assert device.pv_sym_host(3, empty) == 3 and device.pv_sym_host(0, empty) == 3
    assert [device.pv_sym_host(3, SR.pack_row(_one_stone(c))) for c in range(16)] == ONE_STONE


def test_pack_row_is_the_library_layout():
    cells = np.random.RandomState(5).randint(0, 3, (3, 225)).astype(np.int8)
    bl, wh = boards.cells_to_words(cells)
    for i in range(3):
        assert SR.pack_row(cells[i]) == [int(x) for x in bl[i]] + [int(x) for x in wh[i]]


def test_host_function_equals_the_reference_and_is_uniform():
    rows = _rows4096()
    for seed in SEEDS:
        got = np.array([device.pv_sym_host(seed, r) for r in rows])
        want = np.array([SR.sym_of(seed, r) for r in rows])
        assert np.array_equal(got, want)
        counts = np.bincount(got, minlength=8)
        print(f"seed {seed}: counts {' '.join(str(int(x)) for x in counts)}")
        # 512 +- 4.7 sigma: a broken hash fails it, the specified one does not
        assert len(counts) == 8 and counts.min() >= 412 and counts.max() <= 612
    assert len({tuple(SR.sym_of(s, r) for r in rows[:64]) for s in SEEDS}) == 3  # the seed matters


# ---------------------------------------------------------------- the transform
def test_map_back_inverts_the_transform():
    x = np.arange(225) * 3 + 7  # 225 distinct values
    for t in range(8):
        assert np.array_equal(SR.map_back(SR.transform_cells(x, t), t), x)
    assert np.array_equal(SR.transform_cells(x, 0), x)


def test_the_eight_images_are_distinct_and_equal_training_planes():
    import training
    cells = np.zeros(225, np.int8)
    cells[0], cells[14], cells[210] = 1, 2, 1  # distinct corner stones: no symmetry fixes the board
    cells[224] = 0
    cells[17] = 2
    images = [tuple(int(v) for v in SR.transform_cells(cells, t)) for t in range(8)]
    assert len(set(images)) == 8
    planes = boards.planes_from_cells(cells[None])[0]
    for t in range(8):
        want = training._transform_planes(planes, t >> 1, bool(t & 1))
        got = boards.planes_from_cells(np.array(images[t], np.int8)[None])[0]
        assert np.array_equal(got, want), t
        assert images[t].count(1) == 2 and images[t].count(2) == 2  # the side to move is unchanged


def test_wrap_is_the_identity_for_an_equivariant_evaluator_and_not_otherwise():
    from puct_ref import uniform_eval
    cells = tuple(_one_stone(0))
    for seed in SEEDS:
        assert SR.wrap(uniform_eval, seed)(cells, 2) == uniform_eval(list(cells), 2)

    def biased(c, player):  # all the mass on the first empty cell: an orientation bias
        k = list(c).index(0)
        return [1.0 if i == k else 0.0 for i in range(225)], 0.25

    t = SR.sym_of(3, SR.pack_row(cells))
    assert t == 4
    prior, v = SR.wrap(biased, 3)(cells, 2)
    y = SR.transform_cells(cells, t)
    first = int(np.flatnonzero(y == 0)[0])
    onehot = np.zeros(225)
    onehot[first] = 1.0
    assert v == 0.25 and prior == [float(x) for x in SR.map_back(onehot, t)] and prior != biased(cells, 2)[0]
    assert cells[prior.index(1.0)] == 0  # the mass lands on an empty cell of x


# ---------------------------------------------------------------- the Python surface
def test_puct_params_carry_the_flag():
    S = 16
    assert _lib.GZ_PUCT_LEAF_SYM == 8
    plain = device.puct_params(S, 1.6)
    assert type(plain) is _lib.PuctParams and plain.flags == 0  # the default: today's struct
    for kw, cls, other in ((dict(), _lib.PuctParams, 0),
                           (dict(dirichlet_alpha=0.3), _lib.PuctNoiseParams, _lib.GZ_PUCT_ROOT_NOISE),
                           (dict(leaves_per_round=4), _lib.PuctBatchParams, _lib.GZ_PUCT_LEAF_BATCH),
                           (dict(dirichlet_alpha=0.3, leaves_per_round=4), _lib.PuctBatchParams,
                            _lib.GZ_PUCT_ROOT_NOISE | _lib.GZ_PUCT_LEAF_BATCH),
                           (dict(fast_simulations=4), _lib.PuctCapParams, _lib.GZ_PUCT_PLAYOUT_CAP),
                           (dict(fast_simulations=4, dirichlet_alpha=0.3), _lib.PuctCapParams,
                            _lib.GZ_PUCT_PLAYOUT_CAP | _lib.GZ_PUCT_ROOT_NOISE)):
        off = device.puct_params(S, 1.6, 2, 9, **kw)
        on = device.puct_params(S, 1.6, 2, 9, leaf_symmetry=True, **kw)
        assert type(on) is type(off) is cls and ctypes.sizeof(on) == ctypes.sizeof(off)
        assert off.flags == other and on.flags == other | 8
        on.flags = off.flags
        assert bytes(on) == bytes(off)  # nothing but the bit differs
    assert [ctypes.sizeof(c) for c in (_lib.PuctParams, _lib.PuctNoiseParams, _lib.PuctBatchParams,
                                       _lib.PuctCapParams)] == [32, 48, 56, 72]
    # with_leaves and the cap keep it
    sym = device.puct_params(S, 1.6, leaf_symmetry=True)
    assert device.with_leaves(sym, 4).flags == 8 | _lib.GZ_PUCT_LEAF_BATCH
    assert device.with_leaves(device.with_leaves(sym, 4), 1).flags == 8
    assert device.with_leaves(sym, 1) is sym
    noisy = device.puct_params(S, 1.6, dirichlet_alpha=0.3, leaf_symmetry=True)
    assert device.with_leaves(device.with_leaves(noisy, 2), 1).flags == 8 | _lib.GZ_PUCT_ROOT_NOISE
    assert device._with_cap(sym, 4, 0.5).flags == 8 | _lib.GZ_PUCT_PLAYOUT_CAP


def test_workspace_sizes():
    L = _lib.load()
    assert L.gz_puct_sym_bytes(1) == 256 and L.gz_puct_sym_bytes(256) == 256 and L.gz_puct_sym_bytes(257) == 512
    al = lambda x: (x + 255) & ~255  # noqa: E731
    for n in (1, 5, 257, 4096):
        assert L.gz_pv_sym_workspace_bytes(n) == al(L.gz_pv_workspace_bytes(n)) + al(64 * n) + al(n)
    off = device.puct_params(16, 1.6)
    on = device.puct_params(16, 1.6, leaf_symmetry=True)
    assert device._puct_workspace_bytes(L, 5, off) == L.gz_puct_workspace_bytes(5, 16)
    assert device._puct_workspace_bytes(L, 5, on) == L.gz_puct_workspace_bytes(5, 16) + L.gz_puct_sym_bytes(5)
    on4 = device.with_leaves(on, 4)
    assert device._puct_workspace_bytes(L, 100, on4) == \
        L.gz_puct_batch_workspace_bytes(100, 16, 4) + L.gz_puct_sym_bytes(400)


def test_leaf_symmetry_needs_the_puct_search():
    import training
    from ai_agent import AlphaZeroGomokuAI
    from gzero.selfplay import SelfPlayEngine
    with pytest.raises(ValueError, match="leaf_symmetry"):
        SelfPlayEngine(n_slots=4, leaf_symmetry=True)
    with pytest.raises(ValueError, match="leaf_symmetry"):
        AlphaZeroGomokuAI(1, "easy", leaf_symmetry=True)
    with pytest.raises(ValueError, match="leaf_symmetry"):
        training.run_iteration(None, None, 0, leaf_symmetry=True)
    with pytest.raises(ValueError, match="leaf_symmetry"):
        training.main(iterations=0, leaf_symmetry=True)
    with pytest.raises(ValueError):
        device.pv_sym_host(0, [0] * 15)


# ---------------------------------------------------------------- C argument errors
def test_argument_errors_without_gpu():
    L = _lib.load()
    one = ctypes.c_void_p(256)  # (never dereferenced: every call fails before a launch)
    assert L.gz_pv_sym(None, 1, 0, one, None) == -1 and b"gz_pv_sym" in L.gz_last_error()
    assert L.gz_pv_sym(one, 1, 0, None, None) == -1
    assert L.gz_pv_sym(one, -1, 0, one, None) == -1
    assert L.gz_pv_sym(None, 0, 0, None, None) == 0
    assert L.gz_pv_sym_host(0, None) == -1 and b"gz_pv_sym_host" in L.gz_last_error()

    def fwd(w=one, b=one, n=1, lg=one, v=one, pr=one, prior=None, ws=one, prec=_lib.GZ_PV_F16X3):
        return L.gz_pv_forward_sym(w, b, n, None, None, 0, lg, v, pr, prior, ws, prec, None)

    for kw in (dict(w=None), dict(b=None), dict(lg=None), dict(v=None), dict(n=-1), dict(ws=None), dict(prec=7),
               dict(pr=None, prior=one)):
        assert fwd(**kw) == -1, kw
        assert b"gz_pv_forward_sym" in L.gz_last_error(), kw
    assert fwd(n=0, w=None, b=None, lg=None, v=None) == 0
    # the flag adds no argument error of its own and hides none
    p = device.puct_params(100000, 1.6, leaf_symmetry=True)
    assert L.gz_puct_search(None, None, 1, ctypes.byref(p), None, None, None, None, None, None) == -1
    assert b"num_simulations" in L.gz_last_error()
    p = device.puct_params(16, 1.6, leaf_symmetry=True)
    assert L.gz_puct_search(None, None, 1, ctypes.byref(p), None, None, None, None, None, None) == -1
    assert b"bad arguments" in L.gz_last_error()
    assert L.gz_puct_search(None, None, 0, ctypes.byref(p), None, None, None, None, None, None) == 0
