"""-m gpu: the eigen-mode route of the whitening set-up for blocks of more than 256 rows (csrc/eigh_large.hip:
two-sided block Jacobi, rotations on fp64 MFMA) -- against LAPACK, against the host engine, through one whole fit.
Every case takes the route through the LSQAMD_EIGH_LARGE=device knob; the inputs are those of test_gpu_eigh_blocks.

C_SOLVER: see profiles/eigh_large.txt for the worst measured ratio of a defect to max(B eps lambda_max, LAPACK's own);
the bound is about twice that, for other seeds and rounding orders, and stays inside the limit of 16 that
test_gpu_eigh_blocks argues for.  The whitening and fit tolerances are that file's."""
import functools

import numpy as np
import pytest

from tests import gpu_util as gu
from tests.test_gpu_eigh_blocks import EPS, amd, clear_of_floor, cluster, corr, gap, rankdef  # noqa: F401 (amd: fixture)

pytestmark = pytest.mark.gpu
C_SOLVER = 1.0


@pytest.fixture(autouse=True)
def large_route_on_device(monkeypatch):
    monkeypatch.setenv('LSQAMD_EIGH_LARGE', 'device')


# 257: one ragged column; 288: nine column blocks, one rests per step; 320: even count; 513: 17 blocks, the last ragged
@pytest.mark.parametrize('B', [257, 288, 320, 513])
def test_solver_against_lapack(amd, B):
    from lsqfit_amd.whiten import _Block, _device_regulate_eig
    rng = np.random.default_rng(1000 + B)
    mats = [corr(f(rng, B)) for f in (rankdef, gap, cluster)]
    out = _device_regulate_eig(mats, 1e-3, False)                    # (floor form: every mode kept, so every block comes back)
    for A, k in zip(mats, out):
        assert k is not None and 1 <= k['sweeps'] < 30
        lam, V = _Block._to_host(k['lam_dev']), _Block._to_host(k['vec_dev'])
        w, v = np.linalg.eigh(A)
        unit = B * EPS * w[-1]
        eye = np.eye(B)
        got = (np.max(np.abs(lam - w)), np.max(np.abs(A @ V - V * lam)), np.max(np.abs(V.T @ V - eye)))
        ref = (0.0, np.max(np.abs(A @ v - v * w)), np.max(np.abs(v.T @ v - eye)))
        print('B=%d sweeps=%d defect / max(unit, LAPACK):' % (B, k['sweeps']), ['%.3f' % (g / max(unit, r)) for g, r in zip(got, ref)])
        assert np.all(np.diff(lam) >= 0)
        for g, r in zip(got, ref):
            assert g <= C_SOLVER * max(unit, r)


@functools.lru_cache(maxsize=None)
def whitening_inputs(B):
    """two rankdef and two gap blocks clear of the floor (read-only; the gap kind depends on |cut| = 1e-3 only)"""
    rng = np.random.default_rng(7000 + B)
    covs = []
    for f in (rankdef, gap):
        covs += [c for c in (f(rng, B) for _ in range(6)) if clear_of_floor(c, 1e-3)][:2]
    assert len(covs) == 4
    return covs


@pytest.mark.parametrize('cut', [1e-3, -1e-3])
@pytest.mark.parametrize('B', [320, 513])
def test_whitening_against_host_engine(amd, B, cut):
    from lsqfit_amd.whiten import regulate_blocks
    covs = whitening_inputs(B)
    dev = regulate_blocks(covs, cut, want_prec=True, engine='device')
    host = regulate_blocks(covs, cut, want_prec=True, engine='host')
    for d, h in zip(dev, host):
        assert 'Wt_dev' in d and d['tri'] == 0 and 'eig_handed_back' not in d
        assert d['modes'] == h['modes'] and d['nmod'] == h['nmod'] > 0
        assert d['logdet'] == pytest.approx(h['logdet'], rel=1e-11)
        hp = h['Wt'] @ h['Wt'].T
        assert gu.relmax(d['Wt'] @ d['Wt'].T, hp) < 1e-9
        assert gu.relmax(d['prec'], hp) < 1e-9
        assert gu.relmax(d['S'] @ d['S'].T, h['S'] @ h['S'].T) < 1e-9
        assert d.has_S_add() == h.has_S_add() == (cut > 0)
        if cut > 0:
            assert gu.relmax(d['S_add'] @ d['S_add'].T, h['S_add'] @ h['S_add'].T) < 1e-9
        else:
            assert d['modes'] < B and np.all(d['Wt'][:, d['modes']:] == 0.0)


def test_fit_with_device_eigen_whitening(amd):
    """make_cosmix(N=640, P=16, block=320) with rank-deficient block covariances (and noise drawn from them)"""
    from lsqfit_amd import synth
    d = synth.make_cosmix(N=640, P=16, seed=5, block=320)
    rng = np.random.default_rng(55)
    sig = d['yerr']['sdev']
    ymean = synth.cosmix_f(d['x'], d['p_true'])
    blocks = []
    for r0 in range(0, 640, 320):
        s = sig[r0:r0 + 320]
        c = corr(rankdef(rng, 320)) * np.outer(s, s)
        assert clear_of_floor(c, 1e-3)
        w, v = np.linalg.eigh(c)
        ymean[r0:r0 + 320] += v @ (np.sqrt(np.clip(w, 0.0, None)) * rng.standard_normal(320))
        blocks.append((r0, c))
    d = dict(d, ymean=ymean, yerr=dict(sdev=sig, blocks=blocks))
    wd = amd.Whitening(d['ymean'], d['yerr'], *d['prior'], svdcut=1e-3, engine='device')
    wh = amd.Whitening(d['ymean'], d['yerr'], *d['prior'], svdcut=1e-3, engine='host')
    assert all('Wt_dev' in k and k['tri'] == 0 for k in wd.blocks)
    assert wd.nchiv == wh.nchiv and wd.nmod == wh.nmod > 0 and wd.logdet == pytest.approx(wh.logdet, rel=1e-11)
    kw = dict(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=d['prior'], svdcut=1e-3)
    fd = amd.nonlinear_fit(problem=amd.DeviceProblem(d['model'], d['x'], wd), **kw)
    fh = amd.nonlinear_fit(problem=amd.DeviceProblem(d['model'], d['x'], wh), **kw)
    assert gu.relmax(fd.pmean, fh.pmean) < 1e-9 and gu.relmax(fd.cov, fh.cov) < 1e-8
    assert fd.chi2 == pytest.approx(fh.chi2, rel=1e-9) and fd.logGBF == pytest.approx(fh.logGBF, rel=1e-9)
    ref = gu.oracle_fit(d, solver='cholesky', svdcut=1e-3)
    assert gu.relmax(fd.pmean, ref.pmean) < 1e-6 and gu.relmax(fd.cov, ref.cov) < 1e-6


def test_routing(amd, monkeypatch):
    from lsqfit_amd.whiten import regulate_blocks
    c = whitening_inputs(320)[0]
    for knob in ('host', None):                                      # no knob: one 320-row block is outside the measured ranges
        monkeypatch.setenv('LSQAMD_EIGH_LARGE', knob) if knob else monkeypatch.delenv('LSQAMD_EIGH_LARGE')
        d, h = (regulate_blocks([c], 1e-3, engine=e)[0] for e in ('device', 'host'))
        assert 'Wt_dev' not in d and np.array_equal(d['Wt'], h['Wt']) and d['nmod'] == h['nmod']
