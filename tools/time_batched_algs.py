"""Developer tool (GPU): what do the dogleg-family methods buy in the lockstep batch engine at config 5's shape?
128 fits of (4096, 512) -- tests/test_gpu_batched.py make(4096, 512, 128, 20264), the prior-width sweep of bench.py's c5 --
run with each of the four methods the engine has: rounds, device time (HIP events around the whole run), the largest
iteration count and the largest |logGBF - logGBF(lm)| over the fits.  One warm-up run per method (graph capture, first-use
costs), then `repeats` timed ones.

    python tools/time_batched_algs.py [repeats] [N P B]
"""
import sys
import numpy as np
sys.path.insert(0, '.')
import lsqfit_amd
from lsqfit_amd import synth

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N, P, B = (int(v) for v in sys.argv[2:5]) if len(sys.argv) > 4 else (4096, 512, 128)
d = synth.make_cosmix(N=N, P=P, seed=20264, block=0, prior_corr=False)
K = P // 2
pm, ps = d['prior']
z = 0.1 * 10 ** (2.0 * np.arange(B) / max(B - 1, 1))
psb = np.tile(ps, (B, 1))
psb[:, :K] = z[:, None]
pmb = np.tile(pm, (B, 1))
bf = lsqfit_amd.BatchedFits(d['model'], d['x'], d['ymean'], d['yerr'], pmb, psb)
base = None
print('%d fits of (%d, %d); device_ms of %d runs after a warm-up' % (B, N, P, repeats))
print('%-11s %6s %8s %8s  %-30s %s' % ('alg', 'rounds', 'max nit', 'max nfev', 'device_ms', 'max |dlogGBF| vs lm'))
for alg in ('lm', 'dogleg', 'ddogleg', 'subspace2D'):
    bf.run(use_graph=True, alg=alg)
    outs = [bf.run(use_graph=True, alg=alg) for _ in range(repeats)]
    out = outs[-1]
    assert np.all(out['status'] == 0), (alg, out['status'])
    if base is None:
        base = out
    print('%-11s %6d %8d %8d  %-30s %.2e' % (alg, out['rounds'], out['nit'].max(), out['nfev'].max(),
                                            ' '.join('%.2f' % o['device_ms'] for o in outs), np.abs(out['logGBF'] - base['logGBF']).max()))
bf.close()
