"""The C-SVC engine (gcc_amd/svc.py) on the lock-step emulator build: CPU tensors, plain addresses."""
from gcc_amd.svc import SVCEngine

from .emu_driver import emu_lib


def emu_ptr(t):
    return t.data_ptr() if t is not None else None


def emu_engine():
    return SVCEngine(emu_lib(), emu_ptr)
