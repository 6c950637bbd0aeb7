"""The one-term fp16 precision ("f16", GZ_PV_F16) without a GPU: the Python surface, the
library's argument checks and the honesty of the CPU restatement the GPU tests measure
the kernel against (tests/pv_f16_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

import pv_f16_ref as F
from gzero import _lib, boards, device, weights


def test_precision_table():
    assert weights.PRECISIONS == {"fp32": 0, "f16x3": 1, "f16": 2}
    assert (_lib.GZ_PV_FP32, _lib.GZ_PV_F16X3, _lib.GZ_PV_F16) == (0, 1, 2)
    with open(_lib.HERE + "/../../include/gzero.h") as f:
        assert "#define GZ_PV_F16 2" in f.read()


@pytest.mark.parametrize("kw", [{}, {"dirichlet_alpha": 0.3}, {"leaves_per_round": 4}])
def test_puct_params_take_f16(kw):
    p = device.puct_params(16, 1.6, 0, 3, precision="f16", **kw)
    assert p.precision == _lib.GZ_PV_F16
    assert device.with_leaves(p, 2).precision == _lib.GZ_PV_F16
    assert device.puct_params(16, precision="f16x3", **kw).precision == _lib.GZ_PV_F16X3
    assert device.puct_params(16, precision="fp32", **kw).precision == _lib.GZ_PV_FP32
    with pytest.raises(ValueError, match="precision"):
        device.puct_params(16, precision="fp16", **kw)


def test_unknown_precision_strings_are_rejected():
    # (each raises before the library or a GPU is asked for)
    from neural_network import GomokuModel
    with pytest.raises(ValueError, match="precision"):
        device.PVWeights(np.zeros(4, np.float32), precision="half")
    with pytest.raises(ValueError, match="precision"):
        GomokuModel(device="cpu", precision="half")
    assert GomokuModel(device="cpu", precision="f16").precision == "f16"


def test_selfplay_precision_needs_the_puct_search():
    import training
    with pytest.raises(ValueError, match="selfplay_precision"):
        training.run_iteration(None, None, 0, selfplay_precision="f16")
    with pytest.raises(ValueError, match="selfplay_precision"):
        training.run_iteration(None, None, 0, search="reference", selfplay_precision="f16")
    with pytest.raises(ValueError, match="selfplay_precision"):
        training.main(iterations=0, selfplay_precision="f16")
    with pytest.raises(ValueError, match="precision"):
        training.run_iteration(None, None, 0, search="puct", selfplay_precision="half")


def test_library_checks_the_precision():
    L = _lib.load()
    one = ctypes.c_void_p(256)  # (never dereferenced: the checks come first)
    for bad in (3, -1, 7):
        assert L.gz_pv_forward(one, one, 1, None, one, one, None, None, one, bad, None) == -1
        assert b"precision" in L.gz_last_error()
    p = _lib.PuctParams(16, 0, 1.6, 0, 3, 0)
    args = (None, None, 1, ctypes.byref(p), None, None, None, None, None, None)
    assert L.gz_puct_search(*args) == -1 and b"precision" in L.gz_last_error()
    p.precision = _lib.GZ_PV_F16  # accepted: the next check (NULL pointers) fails instead
    assert L.gz_puct_search(*args) == -1 and b"precision" not in L.gz_last_error()


def test_emulation_without_rounding_is_the_network():
    """pv_f16_ref.emulate with every fp16 rounding off is the plain network: within 1e-6 of
    weights.reference_forward (fp32 torch) -- in float64 and in float32."""
    cells = F.board_cells(12, seed=5)
    planes = boards.planes_from_cells(cells)
    for seed in (0, 1):
        sd = weights.init_state_dict(seed)
        ref_lg, ref_v = weights.reference_forward(sd, planes)
        for dt in (torch.float64, torch.float32):
            lg, v, pr = F.emulate(sd, planes, dt, rounding=False)
            assert np.abs(lg - ref_lg).max() < 1e-6, (seed, dt, np.abs(lg - ref_lg).max())
            assert np.abs(v - ref_v).max() < 1e-6
            assert np.abs(pr.sum(1) - 1).max() < 1e-6
        t_lg, t_v, _ = F.torch_fp64(sd, planes)
        assert np.abs(t_lg - ref_lg).max() < 1e-6 and np.abs(t_v - ref_v).max() < 1e-6


def test_emulation_rounds_and_the_boards_are_the_stated_ones():
    cells = F.board_cells(40, seed=0)
    stones = (cells != 0).sum(1)
    assert stones[0] == 0 and list(stones[1:5]) == [1, 1, 1, 1] and stones[5] == 120 and stones[6:].max() <= 119
    assert [int(np.flatnonzero(cells[1 + i])[0]) for i in range(4)] == [0, 14, 210, 224]
    planes = boards.planes_from_cells(cells[:8])
    sd = weights.init_state_dict(0)
    e64 = F.emulate(sd, planes, torch.float64)
    t64 = F.torch_fp64(sd, planes)
    d = np.abs(e64[0] - t64[0]).max()
    assert 1e-6 < d < 1e-3, d  # the fp16 maps are visible, and small at init weights
