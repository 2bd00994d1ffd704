"""Shared by the CPU tests of the device bindings (tests/test_post_bindings_cpu.py, tests/test_train_bindings_cpu.py): host tensors that
report cuda:0, and a stand-in device address.  No test functions here."""
import torch


class OnDev0(torch.Tensor):
    """A host tensor that reports cuda:0: reaches the runners' shape and size checks, which come before any device work."""

    @property
    def device(self):
        return torch.device("cuda", 0)


def d0(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(OnDev0)


DEV = torch.device("cuda", 0)
P = 0x10000            # a 256-byte aligned stand-in address: never dereferenced by the entry points' checks
BSR_ERR_ARG = 1
