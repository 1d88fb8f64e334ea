"""Record a launch plan WITHOUT a device: the library's shape queries are the real ones (they need no GPU), the plan-recording
entry points are stubs that count the ops and keep what they were handed (`MockLib.calls`).  Lets the CPU suite run the engine's second pass --
where every activation address is handed out by the arena and checked against the buffer's declared live range."""
import torch

from iip_uavsal_saliency_amd import _lib as L
from iip_uavsal_saliency_amd import engine as E


class MockLib:
    def __init__(self, real):
        self.real, self.n, self.fills, self.lanes = real, 0, [], []
        self.cur_lane = 0
        # (entry point, arguments) of every recording call in order: a copy of the descriptor for the ops that take one, the
        # plain arguments for guard / fork / join / set_lane / patch_ptr (tools/plan_fingerprint.py)
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("uavsal_plan_add_"):
            def add(plan, *a):
                if name == "uavsal_plan_add_fill":
                    d = a[0]._obj
                    self.fills.append((self.n, int(d.out), int(d.n), self.cur_lane))
                if name in ("uavsal_plan_add_guard", "uavsal_plan_add_fork", "uavsal_plan_add_join"):
                    self.calls.append((name, a))
                else:
                    self.calls.append((name, type(a[0]._obj).from_buffer_copy(a[0]._obj)))
                self.n += 1
                return self.n - 1
            return add
        if name == "uavsal_plan_set_lane":
            def set_lane(plan, lane):
                self.cur_lane = lane
                self.calls.append((name, (lane,)))
                return 0
            return set_lane
        if name == "uavsal_plan_patch_ptr":
            def patch_ptr(plan, *a):
                self.calls.append((name, a))
                return 0
            return patch_ptr
        if name == "uavsal_plan_create":
            return lambda: 1
        if name == "uavsal_plan_error_word":
            return lambda p: 4096
        if name in ("uavsal_plan_enable_lanes", "uavsal_plan_destroy", "uavsal_plan_group_mark", "uavsal_plan_group_enable",
                    "uavsal_plan_group_launches", "uavsal_plan_status"):      # (the prior cache's calls: every run "completed")
            return lambda *a: 0
        return getattr(self.real, name)


HOST_ALIGN = 256        # bytes: what the device allocator guarantees at least (torch's host allocator: 64)


class _AlignedTorch:
    """The engine's `torch` while a plan is recorded on the host: allocations start on HOST_ALIGN bytes, as every device
    allocation does.  The library's shape queries read the ADDRESSES of a descriptor too (a split shadow must start on 128
    bytes: `split_eligible`, csrc/conv_gemm.hip), so on a 64-byte host pointer a GEMM whose input exists only as a shadow was
    refused -- "its input only exists as a split shadow but the GEMM is not eligible" -- for a plan the device records fine.
    Nothing recorded is ever launched, so `empty` / `full` leave the memory untouched (a shadow of a big plan is gigabytes)."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _alloc(shape, dtype, device, zero=False):
        if torch.device(device if device is not None else "cpu").type != "cpu":
            raise RuntimeError("mock_plan records on the host")
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        item = torch.empty(0, dtype=dtype).element_size()
        raw = torch.empty(n * item + HOST_ALIGN, dtype=torch.uint8)
        skip = -raw.data_ptr() % HOST_ALIGN
        t = raw[skip:skip + n * item].view(dtype).view(shape)
        assert t.data_ptr() % HOST_ALIGN == 0
        return t.zero_() if zero else t

    def empty(self, shape, dtype=torch.float32, device=None):
        return self._alloc(shape, dtype, device)

    def zeros(self, shape, dtype=torch.float32, device=None):
        return self._alloc(shape, dtype, device, zero=True)

    def full(self, shape, value, dtype=torch.float32, device=None):
        return self._alloc(shape, dtype, device)


class _NoDevice:
    def __init__(self, d):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def record(model, **kw):
    """(engine, mock library) of a plan recorded on the CPU (activations in host memory, nothing launched)."""
    mock = MockLib(L.load())
    orig_load, orig_dev, orig_torch = L.load, torch.cuda.device, E.torch
    L.load, torch.cuda.device, E.torch = (lambda: mock), _NoDevice, _AlignedTorch()
    try:
        eng = E.Engine(model, "cpu", plan_only=True, **kw)       # sizing pass + placement ...
        eng.plan_only = False                                   # ... then the recording pass against the stubs
        eng._init_on_device(True, resume=True)
    finally:
        L.load, torch.cuda.device, E.torch = orig_load, orig_dev, orig_torch
    return eng, mock
