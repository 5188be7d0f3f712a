"""-m gpu: per-fit data covariances in the batched engine (``lsqamdb_set_data_weights``, ``BatchedFits(per_fit_yerr=)``): the
lockstep route and the one-launch route against the single-fit device path and the oracle, per-fit blocks with both
parities of the weight stride, a floor that binds in one fit, re-weighting a live handle, and the two callers the feature
serves -- ``empbayes_fit`` on the data errors (the reference's eg7) and ``bootstrapped_fits(datalist=)``.

Tolerances are those of tests/test_gpu_batched_trs.py: against the single fit pmean 1e-9, chi2 1e-10, cov 1e-8, logGBF 1e-9,
stopping_criterion equal; against the oracle (solver='cholesky') pmean, chi2/dof and cov 1e-6."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import fit as ofit
from tests import gpu_util as gu
from tests.test_gpu_batched import make

pytestmark = pytest.mark.gpu

EG7 = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'eg7.json')))


@pytest.fixture(scope='module')
def amd():
    import lsqfit_amd
    from lsqfit_amd import _lib
    _lib.load()
    return lsqfit_amd


def exp_fcn(x, p):
    return p[0] * np.exp(-p[1] * x)


def exp_jac(x, p):
    e = np.exp(-p[1] * x)
    return np.stack([e, -p[0] * x * e], axis=1)


def compare(amd, out, bf, model, x, ymeans, errs, priors, p0, oracle=None, svdcut=None, alg=None, tol=None, fits=None):
    """every fit of the batch against ``amd.nonlinear_fit`` of the same inputs, and against the oracle (oracle = (fcn, jac))"""
    kw = {}
    if svdcut is not None:
        kw['svdcut'] = svdcut
    if tol is not None:
        kw['tol'] = tol
    B = len(errs)
    assert np.all(out['status'] == 0)
    for b in (range(B) if fits is None else fits):
        ym = ymeans[b] if np.ndim(ymeans) == 2 else ymeans
        single = amd.nonlinear_fit(data=(x, ym, errs[b]), model=model, prior=priors[b], p0=p0[b],
                                   **dict(kw, **({} if alg is None else dict(alg=alg))))
        cov = bf.cov(b) if bf is not None else out['cov'][b]
        print('fit %d: nit %d (single %d)  pmean %.2e  chi2 %.2e  cov %.2e  logGBF %.2e' % (
            b, out['nit'][b], single.nit, gu.relmax(out['pmean'][b], single.pmean), abs(out['chi2'][b] / single.chi2 - 1),
            gu.relmax(cov, single.cov), abs(out['logGBF'][b] / single.logGBF - 1)))
        assert gu.relmax(out['pmean'][b], single.pmean) < 1e-9
        assert out['chi2'][b] == pytest.approx(single.chi2, rel=1e-10)
        assert gu.relmax(cov, single.cov) < 1e-8
        assert out['logGBF'][b] == pytest.approx(single.logGBF, rel=1e-9)
        assert out['stopping_criterion'][b] == single.stopping_criterion
        if oracle is not None:
            okw = dict(kw, **({} if alg is None else dict(alg=alg)))
            ref = ofit.nonlinear_fit(x, ym, gu.dense_cov(errs[b], ym.size), oracle[0], prior_mean=priors[b][0],
                                     prior_err=priors[b][1], p0=p0[b], jac=oracle[1], solver='cholesky', **okw)
            dof = out['dof'] if np.ndim(out['dof']) == 0 else out['dof'][b]
            assert gu.relmax(out['pmean'][b], ref.pmean) < 1e-6
            assert gu.relmax(cov, ref.cov) < 1e-6
            assert out['chi2'][b] / dof == pytest.approx(ref.chi2 / ref.dof, rel=1e-6)


def per_fit_sdev(sig, B, seed):
    """shared sdev x (0.5, 1, 2, ...) x a seeded per-row factor in [0.8, 1.25]"""
    rng = np.random.default_rng(seed)
    return [sig * 0.5 * 2.0 ** b * rng.uniform(0.8, 1.25, sig.size) for b in range(B)]


# ---- 1. diagonal weights, lockstep route ----------------------------------------------------------------------------
@pytest.mark.parametrize('use_graph', [False, True])
def test_diagonal_weights_lockstep(amd, use_graph):
    """N = 300 is no multiple of 64 or 256; fit 1 starts 0.02 off, so the fits finish in different rounds (masks)"""
    d, pmb, psb = make(300, 8, 3, 71)
    errs = per_fit_sdev(d['yerr'], 3, 5)
    p0 = np.tile(d['p0'], (3, 1))
    p0[1] += 0.02
    bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], None, pmb, psb, per_fit_yerr=errs)
    out = bf.run(p0=p0, use_graph=use_graph)
    print('rounds', out['rounds'], 'graph', out['graph_rounds'], 'nit', out['nit'])
    assert out['rounds'] > 1
    if use_graph:
        assert out['graph_rounds'] >= out['rounds'] - 1 > 0
    compare(amd, out, bf, d['model'], d['x'], d['ymean'], errs, list(zip(pmb, psb)), p0, oracle=(gu.cosmix_fcn, gu.cosmix_jac))
    bf.close()


# ---- 2. diagonal weights through a compiled formula -----------------------------------------------------------------
@pytest.mark.parametrize('one_launch', [None, '0'])
def test_diagonal_weights_compiled_formula(amd, monkeypatch, one_launch):
    """16 parameters (> 12: no normal-equation kernel), N = 300, B = 3: the generated residual / Jacobian kernels read
    wdiag + b * wdiag_stride; with LSQAMD_ONE_LAUNCH_FIT=0 the lockstep rounds are certain"""
    from lsqfit_amd import synth
    if one_launch is not None:
        monkeypatch.setenv('LSQAMD_ONE_LAUNCH_FIT', one_launch)
    d = synth.make_cosmix(N=300, P=16, seed=72, block=0, prior_corr=False)
    names = ['a%d' % k for k in range(8)] + ['w%d' % k for k in range(8)]
    model = amd.expr(' + '.join('a%d*cos(w%d*x)' % (k, k) for k in range(8)), names)
    errs = per_fit_sdev(d['yerr'], 3, 6)
    pm, ps = d['prior']
    pmb, psb = np.tile(pm, (3, 1)), np.tile(ps, (3, 1)) * np.array([0.5, 1.0, 2.0])[:, None]
    p0 = np.tile(d['p0'], (3, 1))
    bf = amd.BatchedFits(model, d['x'], d['ymean'], None, pmb, psb, per_fit_yerr=errs)
    out = bf.run(p0=p0)
    print('rounds', out['rounds'], 'nit', out['nit'])
    if one_launch == '0':
        assert out['rounds'] > 1
    compare(amd, out, bf, model, d['x'], d['ymean'], errs, list(zip(pmb, psb)), p0, oracle=(gu.cosmix_fcn, gu.cosmix_jac))
    bf.close()


# ---- 3. one-launch batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4, 130])
def test_one_launch_batch(amd, monkeypatch, N):
    """a*exp(-b*x), B = 4, per-fit sdev: ONE launch (rounds == 1), and again through the lockstep rounds"""
    rng = np.random.default_rng(30 + N)
    x = np.linspace(1.0, 4.0, N)
    y = exp_fcn(x, np.array([9.3, 0.98])) * (1.0 + 0.01 * rng.standard_normal(N))
    model = amd.expr('a*exp(-b*x)', ['a', 'b'])
    errs = [y * z * rng.uniform(0.8, 1.25, N) for z in (0.005, 0.01, 0.02, 0.04)]
    pmb, psb = np.tile([10.0, 1.0], (4, 1)), np.tile([1.0, 0.1], (4, 1))
    p0 = pmb.copy()
    bf = amd.BatchedFits(model, x, y, None, pmb, psb, per_fit_yerr=errs)
    out = bf.run(p0=p0)
    assert out['rounds'] == 1
    compare(amd, out, bf, model, x, y, errs, list(zip(pmb, psb)), p0, oracle=(exp_fcn, exp_jac))
    monkeypatch.setenv('LSQAMD_ONE_LAUNCH_FIT', '0')
    out2 = bf.run(p0=p0)
    assert out2['rounds'] > 1
    compare(amd, out2, bf, model, x, y, errs, list(zip(pmb, psb)), p0, oracle=(exp_fcn, exp_jac))
    bf.close()


# ---- 4. per-fit blocks ----------------------------------------------------------------------------------------------
LAYOUTS = {'odd': [(0, 64), (71, 40), (111, 17)],       # sum of squares 5985: the unaligned weight stride
           'even': [(0, 64), (71, 40), (111, 18)]}      # 6020: the 16-byte loads stay


def corr_matrix(rng, n, mix=0.2):
    """seeded SPD correlation matrix (1 - mix) I + mix C, C with positive correlations: eigenvalues >= 1 - mix"""
    U = rng.uniform(0.1, 0.9, (n, 2 * n))
    c = U @ U.T
    s = 1.0 / np.sqrt(np.diag(c))
    return (1.0 - mix) * np.eye(n) + mix * c * np.outer(s, s)


def block_errs(sig, layout, B, seed, mix=0.2):
    """per-fit covariances D_b R_b D_b on the layout's blocks, D_b = sdev x (0.5, 1, 2) x a row factor"""
    rng = np.random.default_rng(seed)
    out = []
    for sd in per_fit_sdev(sig, B, seed + 1):
        out.append(dict(sdev=sd, blocks=[(r0, corr_matrix(rng, n, mix) * np.outer(sd[r0:r0 + n], sd[r0:r0 + n]))
                                         for r0, n in layout]))
    return out


_BLK = {}


def block_problem():
    from lsqfit_amd import synth
    if not _BLK:
        _BLK.update(synth.make_cosmix(N=192, P=8, seed=73, block=0, prior_corr=True))
    return _BLK


@pytest.mark.parametrize('alg', ['lm', 'dogleg'])
@pytest.mark.parametrize('prior', ['diagonal', 'dense'])
@pytest.mark.parametrize('layout', ['odd', 'even'])
def test_per_fit_blocks(amd, layout, prior, alg):
    d = block_problem()
    assert sum(n * n for _, n in LAYOUTS[layout]) == (5985 if layout == 'odd' else 6020)
    errs = block_errs(d['yerr'], LAYOUTS[layout], 3, 40)
    pm, pcov = d['prior']
    p0 = np.tile(d['p0'], (3, 1))
    if prior == 'diagonal':
        ps = np.sqrt(np.diag(pcov))
        pmb, psb = np.tile(pm, (3, 1)), np.tile(ps, (3, 1)) * np.array([0.5, 1.0, 2.0])[:, None]
        priors = list(zip(pmb, psb))
        bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], None, pmb, psb, per_fit_yerr=errs)
    else:
        pmb = pm[None, :] + 0.02 * np.random.default_rng(4).standard_normal((3, pm.size)) * np.sqrt(np.diag(pcov))
        priors = [(pmb[b], pcov) for b in range(3)]
        wh = amd.Whitening(d['ymean'], errs[0], pm, pcov)
        bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], None, pmb, None, per_fit_yerr=errs, prior_prec=wh.prior_prec,
                             prior_logdet=wh.logdet - wh.logdet_data)
    out = bf.run(p0=p0, alg=alg, tol=1e-10)
    print(layout, prior, alg, 'rounds', out['rounds'], 'tri', bf.wh.tri)
    compare(amd, out, bf, d['model'], d['x'], d['ymean'], errs, priors, p0, oracle=(gu.cosmix_fcn, gu.cosmix_jac), alg=alg,
            tol=1e-10)
    bf.close()


# ---- 5. a floor that binds for one fit only -------------------------------------------------------------------------
def test_floor_binds_in_one_fit(amd):
    """svdcut = 1e-2; fit 1's 17-row block has two nearly equal rows: the eigen route, and tri = 0 for that block in EVERY fit"""
    d = block_problem()
    errs = block_errs(d['yerr'], LAYOUTS['odd'], 3, 50, mix=0.1)
    r0, n = LAYOUTS['odd'][2]
    rng = np.random.default_rng(51)
    L = np.linalg.cholesky(corr_matrix(rng, n, 0.1))
    L[1] = L[0] + 1e-3 * L[1]
    c = L @ L.T
    s = 1.0 / np.sqrt(np.diag(c))
    sd = errs[1]['sdev'][r0:r0 + n]
    errs[1]['blocks'][2] = (r0, c * np.outer(s, s) * np.outer(sd, sd))
    pm, pcov = d['prior']
    ps = np.sqrt(np.diag(pcov))
    pmb, psb = np.tile(pm, (3, 1)), np.tile(ps, (3, 1))
    p0 = np.tile(d['p0'], (3, 1))
    bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], None, pmb, psb, per_fit_yerr=errs, svdcut=1e-2)
    assert bf.wh.tri[2] == 0
    assert amd.Whitening(d['ymean'], errs[0], svdcut=1e-2).block_arrays()[3][2] == 1      # (fit 0's own block is triangular)
    out = bf.run(p0=p0)
    compare(amd, out, bf, d['model'], d['x'], d['ymean'], errs, list(zip(pmb, psb)), p0, oracle=(gu.cosmix_fcn, gu.cosmix_jac),
            svdcut=1e-2)
    bf.close()


# ---- 6. re-weighting a live handle ----------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [False, True])
def test_reweighting_a_live_handle(amd, blocks):
    if blocks:
        d = dict(block_problem())
        d['prior'] = (d['prior'][0], np.sqrt(np.diag(d['prior'][1])))
        errs_a, errs_b = block_errs(d['yerr'], LAYOUTS['odd'], 3, 60), block_errs(d['yerr'], LAYOUTS['odd'], 3, 61)
        shared = errs_a[1]
    else:
        d, _, _ = make(300, 8, 3, 74)
        errs_a, errs_b = per_fit_sdev(d['yerr'], 3, 7), per_fit_sdev(d['yerr'], 3, 8)
        shared = d['yerr']
    pm, ps = d['prior']
    pmb, psb = np.tile(pm, (3, 1)), np.tile(ps, (3, 1)) * np.array([0.5, 1.0, 2.0])[:, None]
    p0 = np.tile(d['p0'], (3, 1))
    bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], shared, pmb, psb)
    base = bf.run(p0=p0)
    bf.set_data_weights(errs_a)
    out_a = bf.run(p0=p0)
    compare(amd, out_a, bf, d['model'], d['x'], d['ymean'], errs_a, list(zip(pmb, psb)), p0)
    bf.set_data_weights(errs_b)
    out_b = bf.run(p0=p0)
    fresh = amd.BatchedFits(d['model'], d['x'], d['ymean'], None, pmb, psb, per_fit_yerr=errs_b)
    out_f = fresh.run(p0=p0)
    for k in ('pmean', 'chi2', 'logGBF', 'nit'):
        assert np.array_equal(out_b[k], out_f[k]), k
    assert np.array_equal(bf.cov_all(), fresh.cov_all())
    fresh.close()
    # all entries equal: the bits of the shared-weight engine, through the strided reads and after returning to the shared ones
    bf.set_data_weights([shared] * 3)
    same = bf.run(p0=p0)
    assert np.array_equal(same['pmean'], base['pmean']) and np.array_equal(same['chi2'], base['chi2'])
    bf.set_data_weights(None)
    back = bf.run(p0=p0)
    assert np.array_equal(back['pmean'], base['pmean']) and np.array_equal(back['chi2'], base['chi2'])
    assert np.array_equal(back['logGBF'], base['logGBF'])
    bf.close()


# ---- 7. empbayes on the data errors (the reference's eg7) -----------------------------------------------------------
@pytest.mark.parametrize('case', ['eg7a', 'eg7b'])
def test_empbayes_on_data_errors(amd, case):
    """``empbayes_fit(0.001, fitargs, tol=1e-6)`` on the reference's eg7 against the oracle's optimum and the printed results.

    z to 1e-5 relative needs more than the simplex search's stopping rule gives (its vertices within ``tol`` ABSOLUTE of each
    other: eg7a stopped 2.6e-7 = 1.68e-5 relative beside the oracle's optimum, eg7b 1.8e-7 = 2.71e-5, with and without the
    batches); the parabola step that ends a scalar search (sweep.refine_scalar) closes that."""
    from scipy.optimize import minimize_scalar
    from scipy.special import gammaincc
    from lsqfit_amd.sweep import EvidenceSurface
    x, y = np.array(EG7['x']), np.array(EG7['y'])
    pm, ps = np.array(EG7['prior_mean']), np.array(EG7['prior_sdev'])
    k = EG7['cases'][case]
    model = amd.expr('a*exp(-b*x)', ['a', 'b'])

    def dy(z):
        return y * z if k['errors'] == 'relative' else np.ones_like(y) * z

    def fitargs(z):
        return dict(data=(x, y, dy(z)), model=model, prior=(pm, ps))

    def oracle(z):
        return ofit.nonlinear_fit(x, y, dy(z), exp_fcn, prior_mean=pm, prior_err=ps, jac=exp_jac, solver='cholesky')

    fit, z = amd.empbayes_fit(EG7['z0'], fitargs, tol=1e-6)
    surface = EvidenceSurface(fitargs)
    try:
        vals = surface(np.array([[0.5 * z], [z], [2.0 * z]]))
        assert surface.nbatches > 0 and vals.shape == (3,) and int(np.argmin(vals)) == 1
    finally:
        surface.close()
    opt = minimize_scalar(lambda zz: -oracle(zz).logGBF, bounds=(1e-3, 0.1), method='bounded', options=dict(xatol=1e-11))
    ref = oracle(opt.x)
    chi2_dof, Q = fit.chi2 / fit.dof, float(gammaincc(fit.dof / 2.0, fit.chi2 / 2.0))
    print('%s: z %.9g (oracle %.9g, rel %.2e)  logGBF %.9g (oracle %.9g)  p %s sdev %s  chi2/dof %.6g Q %.5g' % (
        case, z, opt.x, abs(z / opt.x - 1), fit.logGBF, ref.logGBF, fit.pmean, fit.psdev, chi2_dof, Q))
    o = k['optimum']
    assert opt.x == pytest.approx(o['z'], rel=2e-5) and ref.logGBF == pytest.approx(o['logGBF'], abs=1e-6)   # (the fixture's note)
    assert fit.dof == k['printed']['dof']
    assert fit.logGBF == pytest.approx(ref.logGBF, abs=1e-6)
    assert gu.relmax(fit.pmean, ref.pmean) < 1e-6
    pr = k['printed']
    if case == 'eg7a':        # every printed figure, at half a unit of its last digit
        assert abs(fit.logGBF - float(pr['logGBF'])) <= 0.5e-4
        assert abs(chi2_dof - float(pr['chi2_dof'])) <= 0.5e-2 and abs(Q - float(pr['Q'])) <= 0.5e-2
        for j in range(2):
            assert abs(fit.pmean[j] - pr['p_mean'][j]) <= 0.5 * pr['p_mean_unit'][j]
            assert abs(fit.psdev[j] - pr['p_sdev'][j]) <= 0.5 * pr['p_sdev_unit'][j]
    else:                     # the reference's search stopped short (the fixture's note): sdev and dy to 2 %
        assert abs(fit.logGBF - float(pr['logGBF'])) <= 2e-4
        for j in range(2):
            assert abs(fit.pmean[j] - pr['p_mean'][j]) <= 0.5 * pr['p_mean_unit'][j]
            assert fit.psdev[j] == pytest.approx(pr['p_sdev'][j], rel=0.02)
        assert z == pytest.approx(pr['dy'], rel=0.02)
    assert z == pytest.approx(opt.x, rel=1e-5)


# ---- 8. bootstrap from a list of data sets --------------------------------------------------------------------------
def scaled_copies(d, n, seed):
    """n data sets: means redrawn around d's, covariance scaled per copy by a seeded factor in [0.7, 1.4]"""
    rng = np.random.default_rng(seed)
    sig = np.asarray(d['yerr']['sdev'] if isinstance(d['yerr'], dict) else d['yerr'], float)
    out = []
    for f in rng.uniform(0.7, 1.4, n):
        ym = d['ymean'] + sig * rng.standard_normal(sig.size)
        if isinstance(d['yerr'], dict):
            ye = dict(sdev=sig * np.sqrt(f), blocks=[(r0, c * f) for r0, c in d['yerr']['blocks']])
        else:
            ye = sig * np.sqrt(f)
        out.append((ym, ye))
    return out


@pytest.mark.parametrize('block', [0, 64])
def test_bootstrap_from_a_datalist(amd, block):
    from lsqfit_amd import synth
    d = synth.make_cosmix(N=300, P=8, seed=77, block=block, prior_corr=False)
    fit = amd.nonlinear_fit(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=d['prior'])
    copies = scaled_copies(d, 6, 9)
    perr = d['prior'][1]
    oracle = (gu.cosmix_fcn, gu.cosmix_jac)

    def check(res, copies, fits=None, with_oracle=()):
        n = len(copies)
        assert res.pmean.shape == (n, 8) and res.prior_means.shape == (n, 8)
        ymeans, errs = [c[-2] for c in copies], [c[-1] for c in copies]
        priors = [(res.prior_means[k], perr) for k in range(n)]
        p0 = np.tile(fit.pmean, (n, 1))
        out = dict(res, status=np.zeros(n, int))
        compare(amd, out, None, d['model'], d['x'], np.array(ymeans), errs, priors, p0, fits=fits)
        if with_oracle:
            compare(amd, out, None, d['model'], d['x'], np.array(ymeans), errs, priors, p0, oracle=oracle, fits=with_oracle)

    res = fit.bootstrapped_fits(datalist=copies, seed=3)
    assert res.engine == 'batched'
    assert np.max(np.abs(res.prior_means - d['prior'][0])) > 0           # redrawn around the fit's prior
    check(res, copies, with_oracle=(0, 5))
    res4 = fit.bootstrapped_fits(n=4, datalist=[(d['x'],) + c for c in copies], seed=3)     # (x, ymean, yerr) entries
    assert res4.engine == 'batched' and res4.pmean.shape == (4, 8)
    assert np.array_equal(res4.prior_means, res.prior_means[:4])
    assert gu.relmax(res4.pmean, res.pmean[:4]) < 1e-9
    # a list whose third copy has another block structure: copy by copy, same numbers
    odd = list(copies)
    ym2, ye2 = copies[2]
    sd2 = np.asarray(ye2['sdev'] if isinstance(ye2, dict) else ye2, float)
    c2 = np.diag(sd2[10:13] ** 2)
    c2[0, 2] = c2[2, 0] = 0.3 * sd2[10] * sd2[12]
    blocks2 = [(10, c2)] if not isinstance(ye2, dict) else [(r0, c) for r0, c in ye2['blocks'] if r0 != 0] + [(10, c2)]
    odd[2] = (ym2, dict(sdev=sd2, blocks=sorted(blocks2, key=lambda t: t[0])))
    res_odd = fit.bootstrapped_fits(datalist=odd, seed=3)
    assert res_odd.engine.startswith('sequential')
    check(res_odd, odd, fits=(1, 2))
    assert gu.relmax(res_odd.pmean[[0, 1, 3, 4, 5]], res.pmean[[0, 1, 3, 4, 5]]) < 1e-9
    # a fit the lockstep engine does not run (solver='qr'): copy by copy with ITS arguments
    fit_qr = amd.nonlinear_fit(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=d['prior'], solver='qr')
    res_qr = fit_qr.bootstrapped_fits(datalist=copies[:2], seed=3)
    assert res_qr.engine.startswith('sequential') and res_qr.pmean.shape == (2, 8)
    assert gu.relmax(res_qr.pmean, res.pmean[:2]) < 1e-6                 # (another solver: the oracle's tolerance)


def test_datalist_of_a_joint_fit_is_refused(amd):
    from lsqfit_amd import synth
    d = synth.make_cosmix(N=40, P=4, seed=78, block=0, prior_corr=False)
    cross = np.zeros((40, 4))
    cross[0, 0] = 0.1 * d['yerr'][0] * d['prior'][1][0]
    fit = amd.nonlinear_fit(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=d['prior'], cross=cross)
    with pytest.raises(NotImplementedError):
        fit.bootstrapped_fits(datalist=[(d['ymean'], d['yerr'])])


# ---- 9. refusals ----------------------------------------------------------------------------------------------------
def hip_runtime():
    """the HIP runtime this process has loaded already (the file behind its mapping: the same library object, not a second copy)"""
    with open('/proc/self/maps') as fh:
        for line in fh:
            if 'libamdhip64' in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError('no HIP runtime mapped')


def test_run_refuses_weights_of_another_batch(amd):
    """weights whose device allocation ends before the last fit's (made for B = 2, the handle runs B = 3): EINVAL from
    lsqamdb_run, nothing launched; wt = NULL although the config has blocks: EINVAL"""
    import torch
    from lsqfit_amd import _lib
    lib = _lib.load()
    d, pmb, psb = make(300, 8, 3, 75)
    bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], d['yerr'], pmb, psb)
    hip = hip_runtime()
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    small = C.c_void_p()
    assert hip.hipMalloc(C.byref(small), 2 * 300 * 8) == 0
    p0 = np.ascontiguousarray(np.tile(d['p0'], (3, 1)))
    try:
        assert lib.lsqamdb_set_data_weights(bf.h, small, None, None) == 0
        rc = lib.lsqamdb_run(bf.h, _lib.dptr(p0), None, 0)
        assert _lib.ERRORS[rc] == 'EINVAL' and b'number of fits' in lib.lsqamdb_last_error(bf.h)
        assert lib.lsqamdb_set_data_weights(bf.h, None, None, None) == 0
        assert lib.lsqamdb_run(bf.h, _lib.dptr(p0), None, 0) == 0           # the shared weights again
    finally:
        bf.close()
        assert hip.hipFree(small) == 0
    dk = block_problem()
    errs = block_errs(dk['yerr'], LAYOUTS['odd'], 3, 62)
    ps = np.sqrt(np.diag(dk['prior'][1]))
    bk = amd.BatchedFits(dk['model'], dk['x'], dk['ymean'], errs[0], np.tile(dk['prior'][0], (3, 1)), np.tile(ps, (3, 1)))
    wd = torch.ones((3, 192), dtype=torch.float64, device=bk.device)
    tri = np.zeros(3, np.int32)
    torch.cuda.synchronize()
    try:
        assert lib.lsqamdb_set_data_weights(bk.h, C.c_void_p(wd.data_ptr()), None, tri.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        p0 = np.ascontiguousarray(np.tile(dk['p0'], (3, 1)))
        rc = lib.lsqamdb_run(bk.h, _lib.dptr(p0), None, 0)
        assert _lib.ERRORS[rc] == 'EINVAL' and b'wt' in lib.lsqamdb_last_error(bk.h)
    finally:
        bk.close()
    with pytest.raises(ValueError, match='3 fits'):
        amd.BatchedFits(dk['model'], dk['x'], dk['ymean'], errs[0], np.tile(dk['prior'][0], (3, 1)),
                        np.tile(ps, (3, 1))).set_data_weights(errs[:2])
