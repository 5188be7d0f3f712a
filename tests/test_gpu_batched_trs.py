"""-m gpu: dogleg, ddogleg and subspace2D steps in the lockstep batch engine (csrc/batch_trs.hip, BatchedFits.run(alg=)):
the symmetric product on the packed tiles alone, the engine against the single-fit device path and the oracle, rejected
trials, blocks + a dense shared prior, a problem without a Gauss-Newton point, and the callers the feature unblocks."""
import ctypes as C

import numpy as np
import pytest

from oracle import fit as ofit
from tests import gpu_util as gu
from tests.test_gpu_batched import make

pytestmark = pytest.mark.gpu

ALGS = ['dogleg', 'ddogleg', 'subspace2D']
EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def amd():
    import lsqfit_amd
    from lsqfit_amd import _lib
    _lib.load()
    return lsqfit_amd


def oracle(d, alg, tol=1e-8, maxit=1000):
    """gu.oracle_fit(d, solver='cholesky') with the method named"""
    return ofit.nonlinear_fit(d['x'], d['ymean'], gu.dense_cov(d['yerr'], d['ymean'].size), gu.cosmix_fcn, prior_mean=d['prior'][0],
                              prior_err=d['prior'][1], p0=d['p0'], tol=tol, jac=gu.cosmix_jac, solver='cholesky', maxit=maxit, alg=alg)


# ---- 1. the product kernel alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 5, 127, 128, 129, 300])
def test_symv_on_packed_tiles(amd, P):
    """y = A u and u^T A u through lsqamdb_op_symv_packed (packs, then the production kernels): one tile, the tile edge, a
    ragged second tile, three tile rows.  Only the upper triangle is read (the lower is NaN), the masked fit's outputs
    keep their sentinel, and a second call returns the same bits (no floating-point atomics).  Bound: the fp64
    summation bound  |fl(sum of n products) - exact| <= n eps sum |products| (to first order) with n <= P, doubled for
    the two-stage sum and once more for the scalar form's second product: 4 P eps (|A| |u|)."""
    import torch
    from lsqfit_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(100 + P)
    B = 3
    A = rng.standard_normal((B, P, P))
    A = A + A.transpose(0, 2, 1)
    u = rng.standard_normal((B, P))
    Aup = A.copy()
    Aup[:, np.tril_indices(P, -1)[0], np.tril_indices(P, -1)[1]] = np.nan
    dev = torch.device('cuda', torch.cuda.current_device())
    dA, du = torch.from_numpy(Aup).to(dev), torch.from_numpy(u).to(dev)
    act = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    outs = []
    for _ in range(2):
        y = torch.full((B, P), -7.5, dtype=torch.float64, device=dev)
        q = torch.full((B,), -7.5, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        rc = lib.lsqamdb_op_symv_packed(C.c_void_p(torch.cuda.current_stream().cuda_stream), P, B, dA.data_ptr(), du.data_ptr(),
                                        act.data_ptr(), y.data_ptr(), q.data_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((y.cpu().numpy(), q.cpu().numpy()))
    (y, q), (y2, q2) = outs
    assert np.array_equal(y, y2) and np.array_equal(q, q2)             # bit-identical
    assert np.all(y[1] == -7.5) and q[1] == -7.5                       # masked: untouched
    for b in (0, 2):
        want = A[b] @ u[b]
        bound = 4 * P * EPS * (np.abs(A[b]) @ np.abs(u[b]))
        err = np.abs(y[b] - want)
        print('P=%d fit %d: max |y - A u| / bound = %.3f, quad err / bound = %.3f' % (
            P, b, np.max(err / bound), abs(q[b] - u[b] @ want) / (4 * P * EPS * (np.abs(u[b]) @ np.abs(A[b]) @ np.abs(u[b])))))
        assert np.all(np.isfinite(y[b])) and np.all(err <= bound)
        assert abs(q[b] - u[b] @ want) <= 4 * P * EPS * (np.abs(u[b]) @ np.abs(A[b]) @ np.abs(u[b]))


# ---- 2. parity with the single-fit path and the oracle ---------------------------------------------------------------
_PARITY = {}


def parity_reference(amd, alg):
    """the six single fits and oracle fits of the parity problem with this method: made once, read-only"""
    if alg not in _PARITY:
        d, pmb, psb = make(512, 32, 6, 51)
        p0 = np.tile(d['p0'], (6, 1))
        p0[3] += 0.02
        singles, refs = [], []
        for b in range(6):
            singles.append(amd.nonlinear_fit(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=(pmb[b], psb[b]),
                                             p0=p0[b], alg=alg, tol=1e-10))
            refs.append(oracle(dict(d, prior=(pmb[b], psb[b]), p0=p0[b]), alg, tol=1e-10))
        _PARITY[alg] = (d, pmb, psb, p0, singles, refs)
    return _PARITY[alg]


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('alg', ALGS)
def test_batched_trs_matches_single_fits_and_oracle(amd, alg, use_graph):
    d, pmb, psb, p0, singles, refs = parity_reference(amd, alg)
    bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], d['yerr'], pmb, psb)
    out = bf.run(p0=p0, use_graph=use_graph, alg=alg, tol=1e-10)
    print(alg, 'rounds', out['rounds'], 'graph', out['graph_rounds'], 'nit', out['nit'], 'nfev', out['nfev'],
          'single nit', [s.nit for s in singles], 'oracle nit', [r.nit for r in refs])
    assert np.all(out['status'] == 0)
    if use_graph:
        assert out['graph_rounds'] >= out['rounds'] - 1 > 0
    for b in range(6):
        single, ref = singles[b], refs[b]
        assert ref.stopping_criterion == 1 and ref.nit == 5         # (the issue's CPU check of the oracle)
        assert gu.relmax(out['pmean'][b], single.pmean) < 1e-9
        assert out['chi2'][b] == pytest.approx(single.chi2, rel=1e-10)
        assert gu.relmax(bf.cov(b), single.cov) < 1e-8
        assert out['logGBF'][b] == pytest.approx(single.logGBF, rel=1e-9)
        assert out['stopping_criterion'][b] == single.stopping_criterion
        assert abs(int(out['nit'][b]) - single.nit) <= max(2, single.nit // 4), (out['nit'][b], single.nit)
        assert gu.relmax(out['pmean'][b], ref.pmean) < 1e-6
        assert gu.relmax(bf.cov(b), ref.cov) < 1e-6
        assert out['chi2'][b] / out['dof'] == pytest.approx(ref.chi2 / ref.dof, rel=1e-6)
    bf.close()


# ---- 3. rejected trials ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ALGS)
def test_batched_trs_rejections_and_maxit(amd, alg):
    """A start 0.3 off in the frequencies of fit 1: most of its trials are rejected (the oracle needs 34 / 33 / 19 of them
    for 10 iterations); a rejected trial only shrinks delta.  pmean to 1e-6, not test 2's 1e-9: the trajectory ends on
    rounding-level accept / reject decisions."""
    d, pmb, psb = make(256, 16, 4, 52)
    bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], d['yerr'], pmb, psb)
    p0 = np.tile(d['p0'], (4, 1))
    p0[1, 8:] += 0.3
    out = bf.run(p0=p0, alg=alg)
    print(alg, 'nit', out['nit'], 'nfev', out['nfev'], 'status', out['status'], 'chi2', out['chi2'])
    assert np.all(out['status'] == 0)
    assert out['nfev'][1] > out['nit'][1] + 1
    for b in range(4):
        single = amd.nonlinear_fit(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=(pmb[b], psb[b]), p0=p0[b], alg=alg)
        ref = oracle(dict(d, prior=(pmb[b], psb[b]), p0=p0[b]), alg)
        assert gu.relmax(out['pmean'][b], single.pmean) < 1e-6
        assert gu.relmax(out['pmean'][b], ref.pmean) < 1e-6
    out = bf.run(p0=p0, alg=alg, maxit=3, tol=1e-14)
    assert np.all(out['nit'] == 3) and np.all(out['status'] == 11)
    bf.close()


# ---- 4. correlated data blocks and a dense prior shared by the fits ---------------------------------------------------------
_BLOCKS = {}


@pytest.mark.parametrize('alg', ALGS)
def test_batched_trs_blocks_and_dense_prior(amd, alg):
    from lsqfit_amd import synth
    if not _BLOCKS:
        d = synth.make_cosmix(N=512, P=32, seed=61, block=64, prior_corr=True)
        pm, perr = d['prior']
        pmb = pm[None, :] + 0.02 * np.random.default_rng(4).standard_normal((3, pm.size)) * np.sqrt(np.diag(perr))
        base = amd.nonlinear_fit(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=d['prior'])
        _BLOCKS.update(d=d, pmb=pmb, wh=base.whitening)
    d, pmb, wh = _BLOCKS['d'], _BLOCKS['pmb'], _BLOCKS['wh']
    perr = d['prior'][1]
    bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], None, pmb, None, whitening=wh, n_fits=3, prior_prec=wh.prior_prec,
                         prior_logdet=wh.logdet - wh.logdet_data)
    out = bf.run(p0=np.tile(d['p0'], (3, 1)), alg=alg, tol=1e-10)
    assert np.all(out['status'] == 0)
    for b in range(3):
        single = amd.nonlinear_fit(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=(pmb[b], perr), p0=d['p0'], alg=alg,
                                   tol=1e-10)
        assert gu.relmax(out['pmean'][b], single.pmean) < 1e-9
        assert out['chi2'][b] == pytest.approx(single.chi2, rel=1e-9)
        assert out['logGBF'][b] == pytest.approx(single.logGBF, rel=1e-9)
        ref = oracle(dict(d, prior=(pmb[b], perr)), alg)
        assert gu.relmax(out['pmean'][b], ref.pmean) < 1e-6
        assert gu.relmax(bf.cov(b), ref.cov) < 1e-6
        assert out['chi2'][b] / out['dof'] == pytest.approx(ref.chi2 / ref.dof, rel=1e-6)
    bf.close()


# ---- 5. no Gauss-Newton point ----------------------------------------------------------------------------------------------
def test_batched_dogleg_without_a_gauss_newton_point(amd):
    """Two identical columns, no prior: J^T J is singular at every point.  The single-fit path's legs_gn takes LSQAMD_ENOTPD from
    the undamped solve as 'no Gauss-Newton point' and stays on the gradient leg (not a failed trial); the batch must do the
    same per fit -- no fault, no hang, and the status, stopping criterion and iteration count of the single fits.
    (Observed: the single-fit path does not error here; both paths end after 3 iterations on the gradient test, status 0.)"""
    rng = np.random.default_rng(9)
    N = 40
    x = np.linspace(0.5, 4.0, N)
    sd = np.full(N, 0.05)
    ym = np.array([1.3 * x + 0.7 + sd * rng.standard_normal(N), -0.4 * x + 2.0 + sd * rng.standard_normal(N)])
    model = amd.expr('a*x + b*x + c', ['a', 'b', 'c'])
    p0 = np.array([0.3, 0.2, 0.1])
    bf = amd.BatchedFits(model, x, ym, sd, None, None, n_fits=2)
    out = bf.run(p0=p0, alg='dogleg', maxit=5, covariance=False)
    bf.close()
    print('batch: nit', out['nit'], 'status', out['status'], 'criterion', out['stopping_criterion'], 'nfev', out['nfev'], 'chi2', out['chi2'])
    for b in range(2):
        single = amd.nonlinear_fit(data=(x, ym[b], sd), model=model, p0=p0, alg='dogleg', maxit=5)
        print('single %d: nit %d criterion %d error %r chi2 %.6g' % (b, single.nit, single.stopping_criterion, single.error, single.chi2))
        assert (out['status'][b] == 11) == (single.error is not None)
        assert out['stopping_criterion'][b] == single.stopping_criterion
        assert out['nit'][b] == single.nit
        assert out['chi2'][b] == pytest.approx(single.chi2, rel=1e-8)


# ---- 6. the callers ----------------------------------------------------------------------------------------------------------
def test_callers_reach_the_engine_with_the_method(amd):
    from lsqfit_amd import synth
    d = synth.make_cosmix(N=300, P=8, seed=77, block=0, prior_corr=False)
    data = (d['x'], d['ymean'], d['yerr'])
    fit = amd.nonlinear_fit(data=data, model=d['model'], prior=d['prior'], alg='dogleg')
    res = fit.bootstrapped_fits(4, seed=3)
    assert res.engine == 'batched'
    for k in range(4):
        single = amd.nonlinear_fit(data=(d['x'], res.ymeans[k], d['yerr']), model=d['model'], prior=(res.prior_means[k], d['prior'][1]),
                                   p0=fit.pmean, alg='dogleg')
        assert gu.relmax(res.pmean[k], single.pmean) < 1e-8 and res.chi2[k] == pytest.approx(single.chi2, rel=1e-8)
    fq = amd.nonlinear_fit(data=data, model=d['model'], prior=d['prior'], alg='dogleg', solver='qr')
    assert fq.bootstrapped_fits(2, seed=3).engine.startswith('sequential')
    widths = [0.2, 0.5, 1.0, 2.0]
    lm = amd.prior_width_sweep(data, d['model'], d['prior'][0], widths, tol=1e-10)
    dd = amd.prior_width_sweep(data, d['model'], d['prior'][0], widths, tol=1e-10, alg='ddogleg')
    for a, b in zip(lm, dd):
        assert b.logGBF == pytest.approx(a.logGBF, rel=1e-8)
        assert gu.relmax(b.pmean, a.pmean) < 1e-6
    pmb = np.tile(d['prior'][0], (2, 1))
    bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], d['yerr'], pmb, np.tile(d['prior'][1], (2, 1)))
    with pytest.raises(RuntimeError, match='EUNSUPPORTED'):
        bf.run(alg='lmaccel')
    with pytest.raises(ValueError):
        bf.run(alg='cgst')
    bf.close()
