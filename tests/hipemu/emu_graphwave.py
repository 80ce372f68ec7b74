"""The GraphWave engine (gcc_amd/graphwave.py) on the lock-step emulator build: CPU tensors, plain addresses."""
from gcc_amd.graphwave import GraphWaveEngine

from .emu_driver import emu_lib
from .emu_logreg import emu_ptr


def emu_engine():
    return GraphWaveEngine(emu_lib(), emu_ptr, "cpu")
