"""Developer tool (GPU): what do per-fit whitening weights (lsqamdb_set_data_weights, BatchedFits(per_fit_yerr=)) cost in
the lockstep batch engine?  Two shapes, each run with the weights shared by the fits and with one set of weights per fit
(the same values B times, so both runs do the same iterations):

  * config 5's shape, 128 fits of (4096, 512), diagonal data covariance -- make(4096, 512, 128, 20264) of
    tests/test_gpu_batched.py, bench.py's c5;
  * 16 fits of (4096, 512) with 256-row covariance blocks.

Per run: rounds, device ms (HIP events around the whole run) and device ms per round; the set-up time of
``stack_whitenings`` per batch (host + device factorisations, weights left in HBM) and of ``set_data_weights``.  One warm-up
run per case (graph capture, first-use costs), then `repeats` timed ones.  ``parent_ms_per_round``: the parent build's
shared-weight c5 figure, for the ratio.

    python tools/time_batched_weights.py [repeats] [parent_ms_per_round]
"""
import sys
import time
import numpy as np
sys.path.insert(0, '.')
import lsqfit_amd
from lsqfit_amd import synth
from lsqfit_amd.whiten import stack_whitenings

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
parent = float(sys.argv[2]) if len(sys.argv) > 2 else None


def timed(bf, label, base=None):
    bf.run(use_graph=True, covariance=False)
    outs = [bf.run(use_graph=True, covariance=False) for _ in range(repeats)]
    out = outs[-1]
    assert np.all(out['status'] == 0), (label, out['status'])
    per = [o['device_ms'] / o['rounds'] for o in outs]
    line = '%-34s rounds %3d  device_ms %s  ms/round %s' % (label, out['rounds'], ' '.join('%.2f' % o['device_ms'] for o in outs),
                                                           ' '.join('%.4f' % v for v in per))
    if base is not None:
        line += '  = %.4f x shared' % (np.median(per) / base)
        assert np.array_equal(out['pmean'], base_out['pmean']), 'per-fit copies of the shared weights must give the shared bits'
    if parent:
        line += '  = %.4f x parent' % (np.median(per) / parent)
    print(line)
    return float(np.median(per)), out


for N, P, B, block in ((4096, 512, 128, 0), (4096, 512, 16, 256)):
    d = synth.make_cosmix(N=N, P=P, seed=20264, block=block, prior_corr=False)
    pm, ps = d['prior']
    psb = np.tile(ps, (B, 1))
    psb[:, :P // 2] = (0.1 * 10 ** (2.0 * np.arange(B) / max(B - 1, 1)))[:, None]
    pmb = np.tile(pm, (B, 1))
    print('%d fits of (%d, %d), %s' % (B, N, P, '%d-row covariance blocks' % block if block else 'diagonal data covariance'))
    bf = lsqfit_amd.BatchedFits(d['model'], d['x'], d['ymean'], d['yerr'], pmb, psb)
    base, base_out = timed(bf, 'shared weights')
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        bw = stack_whitenings(d['ymean'], [d['yerr']] * B)
        t.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    bf.set_data_weights(bw)
    t_set = time.perf_counter() - t0
    print('%-34s %s ms per batch (three calls); set_data_weights %.2f ms' % ('stack_whitenings', ' '.join('%.2f' % (1e3 * v) for v in t),
                                                                           1e3 * t_set))
    timed(bf, 'per-fit weights (strided reads)', base)
    bf.close()
