"""Developer tool (GPU): set-up time of ``Whitening(...)`` with ``svdcut=1e-3`` on rank-deficient sample covariances
(B // 2 samples of B points: every block takes the eigen-mode route), with the eigen-decompositions on the device
(lsqamd_whiten_blocks_eig, csrc/eigh_blocks.hip) against LAPACK on the host, block by block (``LSQAMD_EIGH=host``: the
routing before the device solver existed; ``LSQAMD_EIGH=device`` forces the device route whatever the batch).  Shapes (n_blocks, B): (256, 256) config 4's blocks, (16, 256), (1, 64) and
(512, 48), what ``stack_whitenings`` sees for 128 bootstrap copies of 4 blocks.

Per shape: one warm-up of either route, then `repeats` timed pairs, the two routes ALTERNATING; median and
[min, max] of each, and their ratio.  Then the device call on its own (``lsqamd_whiten_blocks_eig`` through
``_device_regulate_eig``: copy-in, correlation, eigensolver, weights, read-back; a host clock round a call that ends in a
stream synchronise) and the sweeps the solver took.  Last, a crossover scan over (B, n_blocks).

    python tools/time_eigh_blocks.py [repeats]
"""
import os
import sys
import time
import numpy as np
sys.path.insert(0, '.')
import lsqfit_amd
from lsqfit_amd.whiten import _device_regulate_eig

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SHAPES = ((256, 256), (16, 256), (1, 64), (512, 48))


def setup_seconds(ymean, yerr, route):
    os.environ['LSQAMD_EIGH'] = route
    t0 = time.perf_counter()
    wh = lsqfit_amd.Whitening(ymean, yerr, svdcut=1e-3)
    wh.block_arrays()                                  # the weights as the device path takes them (joined in HBM / on the host)
    dt = time.perf_counter() - t0
    assert ('Wt_dev' in wh.blocks[0]) == (route == 'device')
    return dt, wh.logdet, wh.nmod


for nb, B in SHAPES:
    rng = np.random.default_rng(nb * 1000 + B)
    covs = []
    for _ in range(nb):
        X = rng.standard_normal((B // 2, B)) * rng.uniform(0.1, 10.0, B)
        covs.append(np.cov(X, rowvar=False))
    N = nb * B
    yerr = dict(sdev=np.sqrt(np.concatenate([np.diag(c) for c in covs])), blocks=[(b * B, c) for b, c in enumerate(covs)])
    ymean = np.zeros(N)
    n = repeats
    t = dict(host=[], device=[])
    ref = {}
    for route in ('host', 'device'):
        ref[route] = setup_seconds(ymean, yerr, route)[1:]
    assert ref['host'][1] == ref['device'][1] and abs(ref['host'][0] - ref['device'][0]) <= 1e-10 * abs(ref['host'][0])
    for _ in range(n):
        for route in ('host', 'device'):
            t[route].append(setup_seconds(ymean, yerr, route)[0])
    call = []
    for _ in range(n + 1):
        t0 = time.perf_counter()
        blocks = _device_regulate_eig(covs, 1e-3, False)
        call.append(time.perf_counter() - t0)
    sweeps = [k['sweeps'] for k in blocks]
    med = {r: float(np.median(v)) for r, v in t.items()}
    print('(%3d, %3d)  host %9.3f ms [%9.3f, %9.3f]   device %8.3f ms [%8.3f, %8.3f]   device / host %.4f   (%d pairs)'
          % (nb, B, 1e3 * med['host'], 1e3 * min(t['host']), 1e3 * max(t['host']), 1e3 * med['device'], 1e3 * min(t['device']),
             1e3 * max(t['device']), med['device'] / med['host'], n))
    print('            device call alone %8.3f ms [%8.3f, %8.3f]   sweeps min %d median %d max %d'
          % (1e3 * float(np.median(call[1:])), 1e3 * min(call[1:]), 1e3 * max(call[1:]), min(sweeps), int(np.median(sweeps)),
             max(sweeps)), flush=True)

# crossover scan: regulate_blocks (the Cholesky attempt that hands the blocks back included, as in either routing) with the
# handed-back blocks forced to LAPACK / to the device; what EIGH_DEVICE_MIN_BLOCKS in lsqfit_amd/whiten.py is read from
from lsqfit_amd.whiten import regulate_blocks
print('crossover scan: regulate_blocks ms, median of %d alternating pairs' % repeats)
for B in (16, 64, 128, 256):
    rng = np.random.default_rng(B)
    for nb in (1, 4, 16, 64, 256, 1024):
        if nb * B * B > 1 << 24:
            continue
        covs = [np.cov(rng.standard_normal((max(B // 2, 2), B)) * rng.uniform(0.1, 10.0, B), rowvar=False) for _ in range(nb)]
        t = dict(host=[], device=[])
        for it in range(repeats + 1):
            for route in ('host', 'device'):
                os.environ['LSQAMD_EIGH'] = route
                t0 = time.perf_counter()
                regulate_blocks(covs, 1e-3, engine='device')
                if it:
                    t[route].append(time.perf_counter() - t0)
        h, d = float(np.median(t['host'])), float(np.median(t['device']))
        print('  B %3d  n_blocks %4d   host %9.3f [%9.3f, %9.3f]   device %9.3f [%9.3f, %9.3f]   device / host %.3f'
              % (B, nb, 1e3 * h, 1e3 * min(t['host']), 1e3 * max(t['host']), 1e3 * d, 1e3 * min(t['device']),
                 1e3 * max(t['device']), d / h), flush=True)
os.environ.pop('LSQAMD_EIGH', None)
