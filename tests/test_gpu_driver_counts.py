"""-m gpu: what the single-fit host drivers evaluate and exchange, route by route.

A one-rank reduce hook that only counts (the sum over one rank is the identity) takes the one-launch fit and the fused
small-fit kernels out of the way, so the host drivers of lm_driver.hip and scipy_methods.hip run every route; the hook
sees one packed (J^T J | J^T f | chi2) exchange per Jacobian and one scalar per residual evaluation.  Each route must
give the hook-free fit's numbers bit for bit, and its exchanges must stand in the relation to summary.nfev / njev that
the driver's code implies."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 32
NPK = 128 * 128 + P + 1        # the packed 128 x 128 tile of J^T J, then J^T f, then chi2


@pytest.fixture(scope='module')
def amd():
    import lsqfit_amd
    from lsqfit_amd import _lib
    _lib.load()
    return lsqfit_amd


@pytest.fixture(scope='module')
def data():
    # the smallest shape that takes the general multi-kernel path with a correlated block and a dense prior
    from lsqfit_amd import synth
    return synth.make_cosmix(N=512, P=P, seed=41, block=64, prior_corr=True)


# Size-1 exchanges against summary.nfev.  Everywhere the first evaluation is do_init's eval_normal_dev (lm_driver.hip
# do_init: `f->nfev++` after it), which exchanges the packed block and no scalar -- hence the "- 1".
#   nfev-1   every later nfev is one eval_residual_dev (eval.hip eval_residual_dev: `f->nfev++`), whose
#            eval_residual_launch ends in do_reduce(f, f->red_scalar, 1):
#              dogleg / ddogleg / subspace2D and lm under LSQAMD_HOST_LM: lm_driver.hip iterate, the trial residual (the
#                queued lm path takes its `f->nfev--` only on a failed factorisation: chol_fail is asserted 0);
#              trf, dogbox, minpack lm: scipy_methods.hip run_trf / run_dogbox / run_minpack, the trial residual;
#              lm on the device: lm_driver.hip enqueue_trial's eval_residual_launch per trial, iterate_device's
#                `if (st[LMS_SOLVED] != 0.0) f->nfev++` (again: chol_fail is asserted 0).
#   lmaccel  as above, and every trial first evaluates the residual at x + h v through grad_like_at (eval.hip): one
#            more eval_residual_dev (counted in nfev, one scalar) and one exchange of the P-vector J^T r -- so the
#            scalars are still nfev - 1, and there are (nfev - 1) / 2 exchanges of size P.
#   varpro   iterate_varpro evaluates trial points with eval_normal_dev and counts them itself (`f->nfev++` after both
#            calls, and after do_init's second one): packed exchanges only, no scalar at all.
ROUTES = {
    'lm': ('mi355x_lm', dict(alg='lm'), {}, 'nfev-1'),
    'lmaccel': ('mi355x_lm', dict(alg='lmaccel'), {}, 'lmaccel'),
    'dogleg': ('mi355x_lm', dict(alg='dogleg'), {}, 'nfev-1'),
    'ddogleg': ('mi355x_lm', dict(alg='ddogleg'), {}, 'nfev-1'),
    'subspace2D': ('mi355x_lm', dict(alg='subspace2D'), {}, 'nfev-1'),
    'host_lm': ('mi355x_lm', dict(alg='lm'), {'LSQAMD_HOST_LM': '1'}, 'nfev-1'),
    'varpro': ('mi355x_lm', dict(alg='lm', linear=list(range(P // 2))), {}, 'varpro'),
    'trf': ('mi355x_trf', dict(method='trf'), {}, 'nfev-1'),
    'dogbox': ('mi355x_trf', dict(method='dogbox'), {}, 'nfev-1'),
    'minpack_lm': ('mi355x_trf', dict(method='lm'), {}, 'nfev-1'),
}


@pytest.mark.parametrize('route', list(ROUTES))
def test_exchanges_follow_the_evaluation_counts(amd, data, monkeypatch, route):
    fitter, opts, env, relation = ROUTES[route]
    # (a hook-free fit of this size takes fused single-workgroup tails a handle with a hook does not: same arithmetic up to
    #  the order of a few sums; bit-for-bit identity is a statement about the general kernels)
    monkeypatch.setenv('LSQAMD_SMALL_FUSE', '0')
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = data
    kw = dict(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=d['prior'], fitter=fitter, **opts)
    ref = amd.nonlinear_fit(**kw)
    pr = amd.DeviceProblem(d['model'], d['x'], amd.Whitening(d['ymean'], d['yerr'], *d['prior']))
    calls = []
    pr.set_reduce(lambda ptr, count: calls.append(count))
    try:
        fit = amd.nonlinear_fit(problem=pr, **kw)
    finally:
        pr.close()
    s = fit.fitter_results.summary
    print('%s: nit %d nfev %d njev %d ntrial %d chol_fail %d; exchanges packed %d scalar %d size-P %d other %d'
          % (route, s.nit, s.nfev, s.njev, s.ntrial, s.chol_fail, calls.count(NPK), calls.count(1), calls.count(P),
             len(calls) - calls.count(NPK) - calls.count(1) - calls.count(P)))
    assert fit.error is None and ref.error is None
    assert np.array_equal(fit.pmean, ref.pmean) and np.array_equal(fit.cov, ref.cov)
    assert fit.chi2 == ref.chi2 and fit.nit == ref.nit
    assert calls.count(NPK) == s.njev
    assert s.chol_fail == 0
    if relation == 'varpro':
        assert calls.count(1) == 0
        assert s.nfev <= s.njev       # (a pass that gives up re-evaluates the current point without counting it)
    else:
        assert calls.count(1) == s.nfev - 1
    assert calls.count(P) == ((s.nfev - 1) // 2 if relation == 'lmaccel' else 0)
    if relation == 'lmaccel':
        assert (s.nfev - 1) % 2 == 0
    assert len(calls) == calls.count(NPK) + calls.count(1) + calls.count(P)
