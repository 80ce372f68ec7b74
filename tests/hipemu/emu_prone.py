"""The ProNE engine (gcc_amd/prone.py) on the lock-step emulator build: CPU tensors, plain addresses."""
from gcc_amd.prone import ProNEEngine

from .emu_driver import emu_lib
from .emu_logreg import emu_ptr


def emu_engine():
    return ProNEEngine(emu_lib(), emu_ptr, "cpu")
