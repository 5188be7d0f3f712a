"""-m gpu: ``BatchedFits.run(solver='qr')`` -- the Householder TSQR covariance of csrc/batch_qr.hip (fits of up to 32
parameters, two launches per batch) against the oracle's QR route: fp64 Householder on the column-normalised whitened Jacobian
stacked on the prior's rows, R^-1 R^-T and 2 sum log|R_jj|.  Bars: tests/test_gpu_qr.py's (cov 1e-6 of its largest entry, pmean
within 1e-5 psdev), logGBF rel 1e-9 / abs 1e-6."""
import numpy as np
import pytest

from lsqfit_amd.build import QR_CHUNK_ROWS
from tests import gpu_util as gu
from tests.test_gpu_qr import hilbert_like

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    import lsqfit_amd
    from lsqfit_amd import _lib
    _lib.load()
    return lsqfit_amd


def monomials(amd, N, P):
    """c0 + c1 x + ... on [-1, 1] (J does not depend on p) -> model, x, J"""
    x = np.linspace(-1.0, 1.0, N)
    text = ' + '.join(['c0'] + ['c%d*x**%d' % (n, n) for n in range(1, P)])
    return amd.expr(text, ['c%d' % n for n in range(P)]), x, x[:, None] ** np.arange(P)[None, :]


def check(out, cov, refs, fits=(0, 1, 2), pmean_bar=1e-5):
    for b in fits:
        print('fit %d: cov error %.1e, pmean error %.1e psdev' % (b, gu.relmax(cov[b], refs[b].cov),
                                                                np.max(np.abs(out['pmean'][b] - refs[b].pmean) / refs[b].psdev)))
        assert gu.relmax(cov[b], refs[b].cov) < 1e-6
        assert np.array_equal(cov[b], cov[b].T)
        assert np.max(np.abs(out['pmean'][b] - refs[b].pmean) / refs[b].psdev) < pmean_bar
        if out['logGBF'] is not None:
            assert out['logGBF'][b] == pytest.approx(refs[b].logGBF, rel=1e-9, abs=1e-6)


# name: (model, N, P, prior, extras) -- what each shape exercises in the kernel
CASES = {
    'partial_pass': ('mono', 20, 5, None, {}),                     # fewer rows than waves x lanes
    'pass_full': ('mono', 64 - 7, 7, None, {}),                    # N = 64 - P: one wave's pass is exactly full ...
    'pass_full_plus_1': ('mono', 64 - 7 + 1, 7, None, {}),         # ... and one row more
    'widest_panel': ('mono', 100, 32, 'diag', {}),                 # PP = 32, 32 fresh rows per pass
    'width_8_no_prior': ('mono', 40, 8, None, {}),
    'width_16': ('mono', 70, 16, 'diag', {}),
    'width_32_padded': ('mono', 70, 17, 'diag', {}),
    'blocks_dense_prior': ('mono', 320, 7, 'dense', dict(block=64)),   # wave merge, in-kernel prior factor, block-whitened rows
    'two_chunks': ('mono', QR_CHUNK_ROWS + 1, 6, None, {}),        # a ragged second chunk of one row
    'own_scratch': ('mono', 16 * QR_CHUNK_ROWS + 1, 32, 'diag', {}),   # 17 chunk R's of 32 x 32: more than a fit's share of chol_work
    'per_fit_yerr': ('mono', 90, 6, 'diag', dict(per_fit=True)),
    'after_lockstep_rounds': ('mono', 90, 6, 'diag', dict(alg='dogleg')),
    'cosmix': ('cosmix', 200, 8, 'diag', {}),
}


@pytest.mark.parametrize('name', list(CASES))
def test_qr_covariance_of_every_fit_matches_the_oracle(amd, name):
    kind, N, P, prior, extra = CASES[name]
    rng = np.random.default_rng(N + P)
    if kind == 'mono':
        model, x, V = monomials(amd, N, P)
        fcn, jac = (lambda xx, p: V @ p), (lambda xx, p: V)
        truth, sd = rng.standard_normal(P), np.full(N, 0.05)
        perr = np.full(P, 2.0)
    else:
        from lsqfit_amd import synth
        d = synth.make_cosmix(N=N, P=P, seed=5, block=0, prior_corr=False)
        model, x, fcn, jac, truth, sd, perr = d['model'], d['x'], gu.cosmix_fcn, gu.cosmix_jac, d['p_true'], d['yerr'], d['prior'][1]
    yerrs = [sd * (1.0 + 0.5 * b * extra.get('per_fit', False)) for b in range(3)]
    if 'block' in extra:
        n = extra['block']
        C = sd[0] ** 2 * 0.5 ** np.abs(np.subtract.outer(np.arange(n), np.arange(n)))
        yerrs = [dict(sdev=sd, blocks=[(r0, C) for r0 in range(0, N, n)])] * 3
    ym = np.array([fcn(x, truth) + sd * rng.standard_normal(N) for b in range(3)])
    pmb = truth + 0.3 * perr * rng.standard_normal((3, P)) if prior else None
    p0 = truth + 0.01
    kw = dict(per_fit_yerr=yerrs) if extra.get('per_fit') else {}
    if prior == 'dense':
        perr = 4.0 * (0.7 * np.eye(P) + 0.3)
        wh = amd.nonlinear_fit(data=(x, ym[0], yerrs[0]), model=model, prior=(pmb[0], perr)).whitening
        bf = amd.BatchedFits(model, x, ym, None, pmb, None, whitening=wh, n_fits=3, prior_prec=wh.prior_prec,
                             prior_logdet=wh.logdet - wh.logdet_data)
    else:
        bf = amd.BatchedFits(model, x, ym, yerrs[0], pmb, perr if prior else None, n_fits=3, **kw)
    run = dict(p0=p0, tol=1e-10, alg=extra.get('alg', 'lm'))
    chol = bf.run(solver='cholesky', **run)
    out = bf.run(solver='qr', **run)
    cov = bf.cov_all()
    bf.close()
    for key in ('pmean', 'chi2', 'nit'):
        assert np.array_equal(out[key], chol[key]), key
    refs = [gu.oracle_fit(dict(x=x, ymean=ym[b], yerr=yerrs[b], prior=(pmb[b], perr) if prior else (None, None), p0=p0),
                          solver='qr', tol=1e-10, fcn=fcn, jac=jac) for b in range(3)]
    check(out, cov, refs)


@pytest.mark.parametrize('P,prior', [(6, False), (7, True), (8, False), (10, False), (11, False)])
def test_ill_conditioned_batches(amd, P, prior):
    """tests/test_gpu_qr.py's ill-conditioned problems, three data sets per batch: the QR route must hold 1e-6 on cov; what the
    normal equations lose is printed, not asserted.  cond(J D) of the column-normalised Jacobian as numpy computes it is 2.2e3,
    1.2e4, 7.0e4 for P = 6, 7, 8 -- the normal equations still hold 1e-6 there (measured 1.5e-11, 2.0e-9, 5.0e-8) -- so P = 10
    (2.3e6) and P = 11 (1.3e7) are what separates the routes: measured 4.8e-11 and 4.1e-10 on the QR route where the batched
    normal equations lose 2.8e-5 and 2.6e-3.  The reference is reproducible at every size: numpy.linalg.qr on the
    column-normalised matrix and on a row-permuted copy of it agree to 2e-14, 2e-14, 1e-12, 5e-11, 2e-10 of the largest entry.
    pmean is printed, not asserted: the batch's STEPS stay on the damped normal equations (the single-fit path of
    tests/test_gpu_qr.py switches to QR-grade trial steps above P = 8, the batch has none), and at P = 11, cond^2 = 1.7e14,
    they end 1.4e-5 psdev from the oracle's QR trajectory in one fit of three (8.5e-8 and 1.1e-7 in the others; below 1e-7 for
    P <= 10).  The covariance of a linear model does not depend on where the steps end."""
    x, text, V = hilbert_like(P)
    rng = np.random.default_rng(P)
    truth, ysd = rng.standard_normal(P), np.full(x.size, 1e-3)
    ym = np.array([V @ truth + ysd * rng.standard_normal(x.size) for b in range(3)])
    model = amd.expr(text, ['c%d' % n for n in range(P)])
    pri = (np.zeros((3, P)), np.full(P, 1e6)) if prior else (None, None)
    bf = amd.BatchedFits(model, x, ym, ysd, pri[0], pri[1], n_fits=3)
    covs = {}
    for solver in ('cholesky', 'qr'):
        out = bf.run(p0=np.zeros(P), tol=1e-12, solver=solver)
        covs[solver] = bf.cov_all()
    bf.close()
    refs = [gu.oracle_fit(dict(x=x, ymean=ym[b], yerr=ysd, prior=(pri[0][b], pri[1]) if prior else (None, None), p0=np.zeros(P)),
                          solver='qr', tol=1e-12, fcn=lambda xx, p: V @ p, jac=lambda xx, p: V) for b in range(3)]
    Jw = V / ysd[:, None]
    print('P = %d: cond(J D) = %.1e, normal equations lose %s of cov' % (
        P, np.linalg.cond(Jw / np.linalg.norm(Jw, axis=0)), ['%.1e' % gu.relmax(covs['cholesky'][b], refs[b].cov) for b in range(3)]))
    check(out, covs['qr'], refs, pmean_bar=np.inf)


def test_refusals_and_a_rank_deficient_fit_in_the_middle(amd):
    model, x, V = monomials(amd, 80, 33)
    bf = amd.BatchedFits(model, x, np.zeros((2, 80)), np.ones(80), np.zeros((2, 33)), np.ones(33))
    with pytest.raises(RuntimeError, match='up to 32 parameters'):
        bf.run(solver='qr')
    with pytest.raises(ValueError):
        bf.run(solver='svd')
    bf.close()
    # the batch shares one model, so the duplicated term ('c2*y' beside 'c1*x', y = x on the first 20 rows and 2 x on the last 10)
    # is every fit's; the MIDDLE fit's data errors (1e150 on the last 10 rows) leave it the rows on which the two columns are equal
    N = 30
    x = np.linspace(0.1, 1.0, N)
    xy = np.stack([x, np.where(np.arange(N) < 20, x, 2.0 * x)], axis=1)
    model = amd.expr('c0 + c1*x + c2*y', ['c0', 'c1', 'c2'], ['x', 'y'])
    V = np.stack([np.ones(N), xy[:, 0], xy[:, 1]], axis=1)
    rng = np.random.default_rng(3)
    truth, sd = np.array([0.5, -1.0, 0.7]), np.full(N, 0.05)
    yerrs = [sd, np.where(np.arange(N) < 20, sd, 1e150), sd]
    ym = np.array([V @ truth + sd * rng.standard_normal(N) for b in range(3)])
    bf = amd.BatchedFits(model, xy, ym, None, None, None, n_fits=3, per_fit_yerr=yerrs)
    out = bf.run(p0=truth + 0.01, tol=1e-10, solver='qr')
    cov = bf.cov_all()
    bf.close()
    assert np.all(np.isnan(cov[1])) and np.isnan(out['logdet_jtj'][1]) and np.all(np.isnan(out['psdev'][1]))
    refs = {b: gu.oracle_fit(dict(x=xy, ymean=ym[b], yerr=sd, prior=(None, None), p0=truth + 0.01), solver='qr', tol=1e-10,
                             fcn=lambda xx, p: V @ p, jac=lambda xx, p: V) for b in (0, 2)}
    check(out, cov, refs, fits=(0, 2))
