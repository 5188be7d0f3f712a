"""Developer tool (GPU): what does the covariance of a batch of small fits cost by route?

  * ``BatchedFits.run(solver='qr')``: the Householder TSQR covariance (csrc/batch_qr.hip; Jacobian again + two launches);
  * ``solver='cholesky'`` of the same build: potrf -> trtri -> product on the normal equations the lockstep rounds left (the
    built-in cosmix model has no one-launch fit kernel, so these batches run lockstep rounds and the chain is what is timed);
  * what such a batch costs today: B single fits with ``solver='qr'`` one after the other, their covariance phase (qr.hip)
    measured on `singles` fits and scaled to B.

Every figure is device time from HIP events on the stream the work runs on: the batch's 'covar' timer (lsqamdb_timing_get,
LSQAMD_T_COVAR) brackets the launches of ``lsqamdb_covariance``, the single fits' 'covar' phase timer those of their
covariance.  The wall-clock time of the synchronous batched call follows in parentheses.  One warm-up, then three runs.

    python tools/time_batched_qr.py [singles]
"""
import sys
import time
import numpy as np
sys.path.insert(0, '.')
import torch
import lsqfit_amd as amd
from lsqfit_amd import _lib, synth

singles = int(sys.argv[1]) if len(sys.argv) > 1 else 8


def covariance_ms(bf, solver, repeats=3):
    dev, wall = [], []
    for k in range(repeats + 1):
        bf.timing(True)                       # (clears the timers)
        bf.run(tol=1e-10, covariance=False, solver=solver)
        torch.cuda.synchronize()
        ld = np.empty(bf.B)
        t0 = time.perf_counter()
        bf._check(bf.lib.lsqamdb_covariance(bf.h, _lib.dptr(ld), bf.B), 'covariance')
        wall.append((time.perf_counter() - t0) * 1e3)
        ms, n = bf.timings()['covar']
        assert n == 1
        dev.append(ms)
    assert np.all(np.isfinite(ld))
    return ' '.join('%.3f' % t for t in dev[1:]) + '  (wall ' + ' '.join('%.3f' % t for t in wall[1:]) + ')'


for B, N, P in ((128, 256, 10), (1024, 64, 8)):
    d = synth.make_cosmix(N=N, P=P, seed=20270, block=0, prior_corr=False)
    pm, ps = d['prior']
    rng = np.random.default_rng(1)
    pmb = pm + 0.1 * ps * rng.standard_normal((B, P))
    ym = d['ymean'] + d['yerr'] * rng.standard_normal((B, N))
    print('%d fits of (%d, %d)' % (B, N, P))
    bf = amd.BatchedFits(d['model'], d['x'], ym, d['yerr'], pmb, ps)
    fmt = lambda v: ' '.join('%.3f' % t for t in v)
    print('  batched qr (jacobian + reduce + finish)   device ms: %s' % covariance_ms(bf, 'qr'))
    print('  batched cholesky (potrf, trtri, product)  device ms: %s' % covariance_ms(bf, 'cholesky'))
    bf.close()
    per = []
    for b in range(singles + 1):
        wh = amd.Whitening(ym[b], d['yerr'], pmb[b], ps)
        pr = amd.DeviceProblem(d['model'], d['x'], wh)
        pr.timing(True)
        amd.nonlinear_fit(data=(d['x'], ym[b], d['yerr']), model=d['model'], prior=(pmb[b], ps), problem=pr, solver='qr', tol=1e-10)
        torch.cuda.synchronize()
        tm = pr.timings()['covar']
        per.append(tm[0] / max(tm[1], 1))
        pr.close()
    per = per[1:]
    print('  single-fit qr covariance (device, %d fits)       ms per fit: %s -> x %d fits = %.1f ms'
          % (singles, fmt(per), B, float(np.median(per)) * B))
