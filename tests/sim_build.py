"""The one way to build an emulator library of tests/sim/: `make` in that directory (its Makefile holds the flags), then dlopen."""
import ctypes
import os
import subprocess

SIM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim")


def sim_library(name):
    """tests/sim/lib<name>_sim.so, built from sim_<name>.cpp (from sim_main.cpp for "dega") if it is out of date, loaded."""
    so = os.path.join(SIM_DIR, "lib%s_sim.so" % name)
    subprocess.run(["make", "-s", "-C", SIM_DIR, so], check=True)
    return ctypes.CDLL(so)
