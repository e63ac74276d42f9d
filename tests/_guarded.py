"""Guard zones for kernel outputs in GPU tests (not a test module): an output placed PAD elements inside a NaN-filled
device buffer, so that a write before its start or past its end, or an element left unwritten, is seen after the call."""
import numpy as np
import torch

PAD = 64


def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


class Guarded:
    """An output of ``shape`` placed PAD elements inside a NaN-filled buffer."""

    def __init__(self, shape, dtype=torch.float32):
        self.shape = tuple(shape)
        self.n = int(np.prod(self.shape))
        self.buf = torch.full((self.n + 2 * PAD,), float("nan"), dtype=dtype, device=dev())

    @property
    def ptr(self):
        return self.buf.data_ptr() + PAD * self.buf.element_size()

    def numpy(self):
        return self.buf[PAD:PAD + self.n].cpu().numpy().reshape(self.shape)

    def check(self, what):
        whole = self.buf.cpu().numpy()
        assert np.isnan(whole[:PAD]).all(), f"{what}: written before its start"
        assert np.isnan(whole[PAD + self.n:]).all(), f"{what}: written past its end"
        assert np.isfinite(whole[PAD:PAD + self.n]).all(), f"{what}: not every element written / finite"

    def untouched(self):
        """True if the whole buffer, output included, is still NaN (a refused call wrote nothing)."""
        return bool(torch.isnan(self.buf).all())
