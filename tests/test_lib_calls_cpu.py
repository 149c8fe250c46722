"""CPU: the calling helpers of moge_amd._lib that every stateless op goes through - `ptr`, `device_of`, `on` - driven with stand-in objects (no
GPU, no C call).  The GPU half is tests/test_hip_stateless_calls.py."""
import contextlib
import ctypes as C

import pytest
import torch

from moge_amd import _lib as L

CUDA0, CUDA1 = torch.device("cuda", 0), torch.device("cuda", 1)


class Fake:
    """what the helpers read of a tensor"""

    def __init__(self, device, address=0x1000):
        self.device = torch.device(device)
        self.is_cuda = self.device.type == "cuda"
        self._address = address

    def data_ptr(self):
        return self._address


def test_ptr_maps_none_to_null_and_a_tensor_to_its_address():
    assert L.ptr(None) is None
    p = L.ptr(Fake(CUDA0, 0xABC0))
    assert isinstance(p, C.c_void_p) and p.value == 0xABC0
    t = torch.zeros(3)
    assert L.ptr(t).value == t.data_ptr()


def test_device_of_returns_the_common_device_and_skips_none():
    a, b = Fake(CUDA1), Fake(CUDA1)
    assert L.device_of("alignment", a) == CUDA1
    assert L.device_of("alignment", None, a, None, b) == CUDA1
    assert L.device_of("alignment", a, b) is a.device                          # returned as is
    with pytest.raises(ValueError):
        L.device_of("alignment", None, None)                                    # nothing to take a device from


def test_device_of_refuses_a_tensor_off_the_gpu():
    for module in ("alignment", "metrics", "refine"):
        with pytest.raises(RuntimeError, match="GPU tensors only") as e:
            L.device_of(module, Fake(CUDA0), Fake("cpu"))
        assert f"moge_amd.{module} " in str(e.value) and "(no CPU path)" in str(e.value)
    with pytest.raises(RuntimeError, match="GPU tensors only") as e:             # the modules with a host form name it
        L.device_of("mesh", torch.zeros(2), host="moge_amd.io", tensors_only=True)
    assert "moge_amd.mesh " in str(e.value) and "moge_amd.io is the host form" in str(e.value)


def test_device_of_refuses_two_gpus_and_names_both():
    with pytest.raises(ValueError) as e:
        L.device_of("evaluation", Fake(CUDA0), None, Fake(CUDA1))
    assert "cuda:0" in str(e.value) and "cuda:1" in str(e.value) and "moge_amd.evaluation" in str(e.value)


def test_device_of_tensors_only_refuses_other_objects():
    with pytest.raises(ValueError, match="expected torch tensors, got list"):
        L.device_of("mesh", [1, 2], host="moge_amd.io", tensors_only=True)
    with pytest.raises(ValueError, match="expected torch tensors, got Fake"):
        L.device_of("panorama_gpu", Fake(CUDA0), tensors_only=True)


def test_on_enters_the_guard_of_the_device_and_asks_for_its_stream(monkeypatch):
    events = []

    @contextlib.contextmanager
    def guard(dev):
        events.append(("enter", dev))
        try:
            yield
        finally:
            events.append(("exit", dev))

    class Stream:
        cuda_stream = 0x5EED

    def current_stream(device=None):
        events.append(("stream", device))
        return Stream()

    monkeypatch.setattr(torch.cuda, "device", guard)
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    with L.on(CUDA1) as st:
        events.append(("body", st))
    assert events == [("enter", CUDA1), ("stream", CUDA1), ("body", 0x5EED), ("exit", CUDA1)]
    events.clear()
    with pytest.raises(KeyError):                                               # the guard is left when the body raises
        with L.on(CUDA0):
            raise KeyError("x")
    assert events == [("enter", CUDA0), ("stream", CUDA0), ("exit", CUDA0)]
