"""tests/devmem.py, the allocation shim of test_gpu_contents.py, on CPU tensors through
a dummy module: a guard that cannot fail checks nothing."""
import types

import pytest
import torch

import devmem


def _dummy():
    """A module whose functions allocate through its module-level name ``torch``, as the
    gzero wrappers do."""
    m = types.ModuleType("devmem_dummy")
    m.torch = torch
    exec("def make(n, dtype=torch.uint8):\n"
         "    return torch.empty(n, dtype=dtype, device='cpu')\n"
         "def make2(shape):\n"
         "    return torch.empty(shape, dtype=torch.float32)\n"
         "def zeros(n):\n"
         "    return torch.zeros(n, dtype=torch.int32, device='cpu')\n", m.__dict__)
    return m


@pytest.mark.parametrize("pattern", [0x00, 0xFF, 0x3C])
def test_requested_bytes_hold_the_pattern(pattern):
    m = _dummy()
    with devmem.poisoned(pattern, guard_bytes=256, modules=[m]) as mem:
        t = m.make(100)
        f = m.make2((3, 5))
        assert t.shape == (100,) and t.dtype == torch.uint8
        assert f.shape == (3, 5) and f.dtype == torch.float32 and f.is_contiguous()
        assert bytes(t.numpy().tobytes()) == bytes([pattern]) * 100
        assert f.numpy().tobytes() == bytes([pattern]) * 60
        a, b = mem.allocations
        assert (a.nbytes, b.nbytes) == (100, 60)
        assert t.data_ptr() == a.base.data_ptr() and f.data_ptr() == b.base.data_ptr()
        assert a.base.numel() == 100 + 256
        assert a.base[100:].numpy().tobytes() == bytes([devmem.GUARD_BYTE]) * 256
        mem.check()
    assert m.torch is torch  # restored


def test_0xff_is_minus_one_and_nan():
    m = _dummy()
    with devmem.poisoned(0xFF, guard_bytes=64, modules=[m]):
        assert m.make(4, torch.int32).tolist() == [-1] * 4
        for dt in (torch.float16, torch.float32, torch.float64):
            assert bool(torch.isnan(m.make(4, dt)).all())


def test_write_past_the_view_fails_and_names_the_offset():
    m = _dummy()
    with pytest.raises(devmem.GuardError) as e:
        with devmem.poisoned(0x00, guard_bytes=128, modules=[m]) as mem:
            m.make(100)
            mem.allocations[0].base[100] = 7  # one byte past the view
            with pytest.raises(devmem.GuardError) as inner:
                mem.check()
            assert "offset 100 " in str(inner.value) and "(0 past its end)" in str(inner.value)
            assert "<string>:2" in str(inner.value)  # the allocating call site, file:line
        # leaving the context checks once more
    assert "offset 100 " in str(e.value)
    assert m.torch is torch


def test_last_guard_byte_is_watched():
    m = _dummy()
    with devmem.poisoned(0xFF, guard_bytes=128, modules=[m]) as mem:
        m.make(8, torch.float32)
        a = mem.allocations[0]
        a.base[32 + 127] = 0
        with pytest.raises(devmem.GuardError, match=r"offset 159 \(127 past its end\)"):
            mem.check()
        a.base[32 + 127] = devmem.GUARD_BYTE
        mem.check()


def test_write_inside_the_view_passes():
    m = _dummy()
    with devmem.poisoned(0xFF, guard_bytes=128, modules=[m]) as mem:
        t = m.make(100)
        t[:] = 3
        t[99] = 0xA4
        mem.check()


def test_leftover_leaves_the_contents_alone():
    m = _dummy()
    with devmem.poisoned(0x00, guard_bytes=64, modules=[m]) as big:
        t = m.make(200)
        t.copy_(torch.arange(200, dtype=torch.uint8))
    with devmem.poisoned(devmem.LEFTOVER, guard_bytes=64, reuse=big, modules=[m]) as small:
        s = m.make(50)
        assert s.data_ptr() == t.data_ptr()
        assert s.tolist() == list(range(50))
        assert len(small.reused()) == 1
        # the guard moved up behind the smaller size, over the larger call's bytes
        assert small.allocations[0].base[50:50 + 64].tolist() == [devmem.GUARD_BYTE] * 64
        assert t[114:].tolist() == list(range(114, 200))
        # a request larger than what the site had before gets a fresh buffer
        assert m.make(4096).data_ptr() != t.data_ptr()
        small.check()


def test_zeros_stays_zeros_and_other_names_forward():
    m = _dummy()
    with devmem.poisoned(0xFF, guard_bytes=64, modules=[m]) as mem:
        z = m.zeros(16)
        assert z.tolist() == [0] * 16
        assert mem.allocations == []
        assert m.torch.float32 is torch.float32 and m.torch.cuda is torch.cuda
        assert isinstance(z, m.torch.Tensor)


def test_patches_the_gzero_modules():
    import importlib
    mods = [importlib.import_module(n) for n in devmem.MODULES]
    with devmem.poisoned(0xFF, guard_bytes=64) as mem:
        assert all(mod.torch is mem.torch for mod in mods)
    assert all(mod.torch is torch for mod in mods)


def test_bad_pattern():
    with pytest.raises(ValueError):
        devmem.Poisoned(256)
    with pytest.raises(ValueError):
        devmem.Poisoned("stale")
