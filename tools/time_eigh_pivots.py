"""Developer tool (GPU): device time of the two inner solves of csrc/eigh_large.hip on their own, on the same 64 x 64
matrices -- eigh_twosided_kernel through lsqamd_op_eigh_pivots, eigh_jacobi_kernel (one-sided, csrc/eigh_blocks.hip) through
the whitening route at 64 rows -- from the kernel tracer, the two ALTERNATING, median of `repeats` after one warm-up.
Matrices: singular correlation matrices (32 samples of 64 points).

    python tools/time_eigh_pivots.py [repeats] [n_matrices ...]      e.g.  5 1 256
"""
import ctypes as C
import os
import sys

import numpy as np
import torch
from torch.profiler import ProfilerActivity, profile

sys.path.insert(0, '.')
from lsqfit_amd import _lib
from lsqfit_amd.whiten import _device_regulate_eig

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
counts = [int(v) for v in sys.argv[2:]] or [1, 256]
os.environ['LSQAMD_EIGH'] = 'device'
lib = _lib.load()


def traced(fn, name):
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
               for e in prof.key_averages() if name in e.key)


for nb in counts:
    rng = np.random.default_rng(nb)
    covs = [np.cov(rng.standard_normal((32, 64)) * rng.uniform(0.1, 10.0, 64), rowvar=False) for _ in range(nb)]
    sd = [np.sqrt(np.diag(c)) for c in covs]
    stack = torch.from_numpy(np.stack([c / np.outer(s, s) for c, s in zip(covs, sd)])).cuda()
    lam = torch.empty((nb, 64), dtype=torch.float64, device='cuda')
    sweeps, status = (torch.zeros(nb, dtype=torch.int32, device='cuda') for _ in range(2))

    def twosided():
        a = stack.clone()
        rc = lib.lsqamd_op_eigh_pivots(None, 64, nb, C.c_void_p(a.data_ptr()), 64, 4096, C.c_void_p(lam.data_ptr()),
                                       C.c_void_p(sweeps.data_ptr()), C.c_void_p(status.data_ptr()))
        assert rc == 0

    words = []
    t = dict(two=[], one=[])
    for it in range(repeats + 1):
        a = traced(twosided, 'eigh_twosided_kernel')
        b = traced(lambda: _device_regulate_eig(covs, 1e-3, False, words), 'eigh_jacobi_kernel')
        if it:
            t['two'].append(a)
            t['one'].append(b)
    print('n_matrices %4d   two-sided %9.1f us [%9.1f, %9.1f] sweeps %s status %s   one-sided %9.1f us [%9.1f, %9.1f] sweeps %s status %s'
          % (nb, np.median(t['two']), min(t['two']), max(t['two']), sorted(set(sweeps.cpu().tolist())), sorted(set(status.cpu().tolist())),
             np.median(t['one']), min(t['one']), max(t['one']), sorted(set(words[-1][0].tolist())), sorted(set(words[-1][1].tolist()))),
          flush=True)
