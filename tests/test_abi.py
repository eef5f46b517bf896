"""The C-ABI shared library must load on a machine WITHOUT a GPU and export every symbol
include/epievo_mi355x.h declares; the product has no CPU fallback, so creating a context
here must fail cleanly rather than route elsewhere."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import pytest

from epievo_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _gpu_present():
    """whether torch sees a GPU, asked in a child process: torch brings its own HIP runtime, and
    initialising it in this process before the product's libraries open the device leaves every
    later context of the suite without one"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(int(torch.cuda.is_available()))"],
                       capture_output=True, text=True, check=True)
    return r.stdout.split()[-1] == "1"


def _declared(header="epievo_mi355x.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(epv_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_build.HIP_SO), "run __graft_entry__.build() first"
    L = ctypes.CDLL(_build.HIP_SO)
    names = _declared()
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    from epievo_amd.sampler import ABI_SYMBOLS
    assert sorted(ABI_SYMBOLS) == names


def test_exchange_library_exports_every_declared_symbol():
    """include/epievo_mi355x_comm.h -> libepv_rccl.so (links librccl; loads without a GPU)"""
    assert os.path.exists(_build.COMM_SO), "run __graft_entry__.build() first"
    L = ctypes.CDLL(_build.COMM_SO)
    names = _declared("epievo_mi355x_comm.h")
    assert len(names) >= 12
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    # no device here: setting up ranks fails cleanly (no fallback transport for a missing GPU)
    if not _gpu_present():
        comms = (ctypes.c_void_p * 2)()
        devs = (ctypes.c_int * 2)(0, 0)
        assert L.epv_comm_init_all(2, devs, comms) != 0


def test_no_cpu_fallback():
    if _gpu_present():
        pytest.skip("a GPU is present")
    from epievo_amd.sampler import DeviceSampler
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        DeviceSampler(0)


def test_product_does_not_import_the_oracle():
    """only tests/, smoke() and bench.py's cpu_baseline may touch oracle/"""
    pkg = os.path.join(ROOT, "epievo_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hpp", ".cpp", ".hip")) and f != "_build.py":
                text = open(os.path.join(dirpath, f)).read()
                for needle in ("liborc", "import orc", "from orc", '#include "orc', "libepievo_ref", "dlopen"):
                    assert needle not in text, (f, needle)
