"""The logistic-regression engine (gcc_amd/logreg.py) on the lock-step emulator build: CPU tensors, plain addresses."""
from gcc_amd.logreg import LogRegEngine

from .emu_driver import emu_lib


def emu_ptr(t):
    return t.data_ptr() if t is not None else None


def emu_engine():
    return LogRegEngine(emu_lib(), emu_ptr)
