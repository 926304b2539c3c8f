"""What the tests of the "many MCMC steps in one launch" runs share (tests/test_*_run*_host.py, tests/test_gpu_*_run*.py,
the replica-exchange tests): the launch counter, the header text the declarations are looked up in, the stand-in
address of the host checks, and the exact comparison of two runs' dictionaries."""
import ctypes as C
import re

import numpy as np
import torch

from l2hmc_amd import _lib

PTR = 16          # any non-NULL address: host checks only


def count_launches(cls, run):
    """The number of kernel launches of profile class `cls` that `run()` makes (l2hmc_profile_begin / _end)."""
    Lh = _lib.lib()
    _lib.check(Lh.l2hmc_profile_begin(cls))
    run()
    ms, n = C.c_double(), C.c_int64()
    _lib.check(Lh.l2hmc_profile_end(C.byref(ms), C.byref(n)))
    return int(n.value)


def header_text(comments=False):
    """The C header with every run of white space as one blank; `comments=False`: with the comments taken out first."""
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    return re.sub(r"\s+", " ", text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def assert_same_run(a, b, keys, what):
    """Two runs' dictionaries hold the same float32 arrays under `keys`, the same final state and the same mean accept
    probability, bit for bit."""
    for k in keys:
        assert a[k].dtype == b[k].dtype == np.float32 and a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k] - b[k]).max()))
    assert torch.equal(a["samples_out"], b["samples_out"]), what
    assert a["mean_accept"] == b["mean_accept"], what
