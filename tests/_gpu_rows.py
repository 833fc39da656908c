"""Device operands of the tests that call the C ABI directly (test_gpu_point_rows.py, test_gpu_loss_rows.py,
test_gpu_lift_index.py, test_gpu_bn_rows.py, test_gpu_misc2d.py, test_gpu_spconv_rows.py): pitched views into wider buffers whose padding is NaN for inputs and a sentinel, which
must survive, for outputs.  No tests here; importing this needs no GPU."""
import numpy as np
import torch

SENTINEL = -12345.0


def dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


def abi():
    from mm2d3d_amd import _lib

    return _lib.lib(), _lib


DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "u8": torch.uint8}
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.uint8: torch.uint8}


class Rows:
    """An [n, c] operand on the device: a view, rows ``ld`` apart, ``off`` elements into a wider flat buffer that holds ``fill``
    everywhere else (before the first row, between rows, behind the last one).  ``dtype``: torch.float32 (default), bfloat16 or
    float16 (or "fp32" / "bf16" / "fp16"; "u8": bytes, such as the max-pool's taps); data and fill are rounded to it (nearest even).  ``tight``: the buffer ends with the last
    element of the last row (a channel slice that reaches the end of its allocation)."""

    def __init__(self, data, n, c, ld, off=0, fill=float("nan"), dtype=torch.float32, tight=False):
        assert c <= ld
        dtype = DTYPES.get(dtype, dtype)
        flat = torch.full((off + (n - 1) * ld + c if tight and n else off + n * ld + 8,), fill, dtype=dtype)
        self._cpu_view = flat.as_strided((n, c), (ld, 1), off)
        if data is not None:
            self._cpu_view.copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(n, c).float())
        self.flat = flat.to(dev())
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat.as_strided((n, c), (ld, 1), off)
        self.ptr = self.flat.data_ptr() + self.flat.element_size() * off
        self.fill = fill
        self._fill_bits = torch.full((1,), fill, dtype=dtype).view(_BITS[dtype]).item()  # NaN compares unequal to itself: compare bits

    def get(self):
        return self.view.cpu().double().numpy()

    def get32(self):
        """The values as they are: float32 (every 16-bit value is one), signed zeros and NaN payloads included."""
        return self.view.cpu().float().numpy()

    def bits(self):
        """The rows as the integers that hold them (int32 / int16)."""
        return self.view.cpu().contiguous().view(_BITS[self.flat.dtype]).numpy()

    def padding_untouched(self):
        chk = self.flat.clone()
        chk.as_strided(self.view.shape, self.view.stride(), self.view.storage_offset()).fill_(self.fill)
        return bool((chk.view(_BITS[chk.dtype]) == self._fill_bits).all())

    def untouched(self):
        """Nothing was written at all: the whole buffer, rows included, still holds the fill value."""
        return bool((self.flat.view(_BITS[self.flat.dtype]) == self._fill_bits).all())


def vec(data, n=None, fill=SENTINEL):
    """A dense vector (or matrix, flattened) between two runs of sentinels."""
    n = int(np.size(data)) if n is None else n
    return Rows(None if data is None else np.asarray(data, np.float64).reshape(1, n), 1, n, n, off=4, fill=fill)


class Ints:
    """A dense integer vector on the device between two runs of ``fill`` (4 elements before, 8 behind)."""

    def __init__(self, data, n=None, dtype=torch.int32, fill=-7):
        n = int(np.size(data)) if n is None else n
        flat = torch.full((4 + n + 8,), fill, dtype=dtype)
        if data is not None:
            flat[4: 4 + n] = torch.from_numpy(np.ascontiguousarray(data).reshape(n)).to(dtype)
        self.flat, self.n, self.fill = flat.to(dev()), n, fill
        self.ptr = self.flat.data_ptr() + 4 * self.flat.element_size()

    def get(self):
        return self.flat[4: 4 + self.n].cpu().numpy()

    def padding_untouched(self):
        f = self.flat.cpu()
        return bool((f[:4] == self.fill).all() and (f[4 + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.flat == self.fill).all())


def ints(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev())
