"""Developer tool (GPU): the eigen-mode route for handed-back blocks of more than 256 rows, on the device
(lsqamd_whiten_blocks_eig -> csrc/eigh_large.hip, through ``_device_regulate_eig``: copy-in, correlation, eigensolver,
weights, read-back) against LAPACK on the host (``_regulate_block(force_eig=True)``, block by block, as ``regulate_blocks``
calls it).  Inputs: rank-deficient sample covariances (B // 2 samples of B points), svdcut = 1e-3.

Per (B, n_blocks): one warm-up of either route, then `repeats` timed pairs, the two routes ALTERNATING; median and
[min, max] of each, their ratio, the sweeps and status words the solver returned (handed-back blocks included), how many blocks were handed
back, and from one further traced call the device time of the inner solves, the rotations and all other kernels.  What
``whiten.EIGH_LARGE_DEFAULT`` is read from.

    python tools/time_eigh_large.py [repeats] [B:nb,nb,... ...]      e.g.  3 512:1,4,16 4096:1
"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
import lsqfit_amd  # noqa: F401
from lsqfit_amd.whiten import _device_regulate_eig, _regulate_block

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
shapes = sys.argv[2:] or ['512:1,4,16', '1024:1,4,16', '2048:1,4,16', '4096:1,4,16', '8192:1,4,16']


def kernel_split(covs):
    """one more device call under the kernel tracer: device time (ms) of the inner solves (eigh_twosided_kernel, or
    eigh_jacobi_kernel under LSQAMD_EIGH_LARGE_INNER=onesided), of the
    rotations (rotate_kernel, both roles) and of every other kernel of the call"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _device_regulate_eig(covs, 1e-3, False)
        torch.cuda.synchronize()
    t = dict(inner=0.0, rot=0.0, other=0.0)
    for e in prof.key_averages():
        us = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
        t['inner' if 'eigh_jacobi_kernel' in e.key or 'eigh_twosided_kernel' in e.key else 'rot' if 'rotate_kernel' in e.key else 'other'] += us
    return tuple('%.2f ms' % (1e-3 * t[k]) for k in ('inner', 'rot', 'other'))


for spec in shapes:
    B, nbs = int(spec.split(':')[0]), [int(v) for v in spec.split(':')[1].split(',')]
    rng = np.random.default_rng(B)
    pool = [np.cov(rng.standard_normal((B // 2, B)) * rng.uniform(0.1, 10.0, B), rowvar=False) for _ in range(max(nbs))]
    for nb in nbs:
        covs = pool[:nb]
        t = dict(host=[], device=[])
        for it in range(repeats + 1):
            t0 = time.perf_counter()
            for c in covs:
                _regulate_block(c, 1e-3, force_eig=True)
            t1 = time.perf_counter()
            words = []
            blocks = _device_regulate_eig(covs, 1e-3, False, words)
            t2 = time.perf_counter()
            if it:
                t['host'].append(t1 - t0)
                t['device'].append(t2 - t1)
        sweeps, status = (np.concatenate(w) for w in zip(*words))      # the solver's words, handed-back blocks included
        split = kernel_split(covs)
        h, d = float(np.median(t['host'])), float(np.median(t['device']))
        print('B %4d  n_blocks %2d   host %10.2f ms [%10.2f, %10.2f]   device %10.2f ms [%10.2f, %10.2f]   device / host %.3f'
              '   sweeps %s   solver status %s   handed back %d   inner solves %s   rotations %s   other kernels %s' % ((B, nb, 1e3 * h, 1e3 * min(t['host']), 1e3 * max(t['host']), 1e3 * d,
                                                 1e3 * min(t['device']), 1e3 * max(t['device']), d / h,
                                                 sorted(set(sweeps.tolist())), sorted(set(status.tolist())),
                                                 sum(k is None for k in blocks)) + split), flush=True)
