"""TEST INFRASTRUCTURE ONLY: the inputs of tests/test_gpu_phasefix_kernels.py (and of the float32 measurement in
tests/test_host_phasefix_ref.py).  (n, source length, hop) -> the seed of phasefix_ref.stems whose stems leave no ambiguous bin
(phasefix_ref.ambiguous_bins == 0 with every weight 0.37, so with any weight table): found on the CPU, asserted where they are used."""
import functools

import numpy as np

from tests import phasefix_ref as R

SHAPES = (1, 511, 512, 513, 2047, 2048, 2049, 3000, 5121)      # at hop 512; 5121 also at hops 256 and 1024
SEEDS = {(1, 1, 512): 3, (511, 511, 512): 0, (512, 512, 512): 0, (513, 513, 512): 0, (2047, 2047, 512): 0, (2048, 2048, 512): 0,
         (2049, 2049, 512): 0, (3000, 3000, 512): 0, (5121, 5121, 512): 1, (5121, 5121, 256): 1,
         (1, 1, 1024): 3, (511, 511, 1024): 0, (512, 512, 1024): 0, (513, 513, 1024): 0, (2047, 2047, 1024): 0, (2048, 2048, 1024): 0,
         (2049, 2049, 1024): 0, (3000, 3000, 1024): 0, (5121, 5121, 1024): 0,
         # a source shorter and longer than the target; the pooled jobs
         (3000, 1, 512): 0, (3000, 1700, 512): 1, (3000, 3777, 512): 0, (2049, 1749, 1024): 0, (700, 1500, 256): 0, (4100, 4100, 512): 0}
ALL_037 = np.full(R.NB, 0.37, np.float32)


def weight_tables():
    """name -> float32 [1025]: the default ramp at 44100 Hz, all 0.37, all 1, all 2 and a negative value"""
    return {"ramp": R.bin_weights(44100), "0.37": ALL_037, "1": np.ones(R.NB, np.float32), "2": np.full(R.NB, 2.0, np.float32),
            "-0.6": np.full(R.NB, -0.6, np.float32)}


@functools.lru_cache(maxsize=None)
def case(n, m, hop):
    """(target [2, n], source [2, m]) float32, read-only"""
    t, s = R.stems(SEEDS[(n, m, hop)], n, m)
    t.setflags(write=False)
    s.setflags(write=False)
    return t, s


@functools.lru_cache(maxsize=None)
def unambiguous(n, m, hop):
    return R.ambiguous_bins(*case(n, m, hop), ALL_037, hop) == 0


@functools.lru_cache(maxsize=None)
def reference(n, m, hop, wname):
    r = R.phase_fix(*case(n, m, hop), weight_tables()[wname], hop)
    r.setflags(write=False)
    return r
